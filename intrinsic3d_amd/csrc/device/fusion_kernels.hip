// TSDF fusion kernels (the stage in front of the path).  Compiled with -ffp-contract=off: allocation and
// integration take discrete decisions on float values (voxel rounding, pixel rounding, truncation tests), so every expression is
// evaluated in the reference's operation order without FMA contraction.
//   SparseVoxelGrid<Voxel>::alloc / integrate            sparse_voxel_grid.cpp:301-467
//   erodeDiscontinuities / computeVertexMap / computeNormals   rgbd/processing.cpp:49-127,184-232
//   SDFAlgorithms::correctSDF                             sdf/algorithms.cpp:260-331
// The reference's map is replaced by an open-addressing table in HBM (64-bit packed keys, linear probing).  What the reference derives
// from its map — the order in which voxels were first inserted, hence the unordered_map iteration order of the saved volume and of
// correctSDF's in-place sweep — is carried by a per-voxel insertion rank that allocation maintains with atomicMin.
#include "fusion_kernels.hpp"
#include "fusion_hash.hpp"
#include "point_cell_device.hpp"      // cell_of_point and the cell of cell_device.hpp: the general merge samples src through them

namespace i3d {
namespace {

constexpr int TPB = 256;

using namespace fusion_hash;          // pack_key, unpack_key, slot_of, find_slot (fusion_hash.hpp)

__device__ inline int round_trunc(float v) { return (int)(v + 0.5f); }                                   // mat.h:90
// pose.topLeftCorner<3,3>() * p + pose.topRightCorner<3,1>() (sparse_voxel_grid.cpp:328,425,584): a fixed-size Eigen product, every coefficient
// the halving reduction a0 + (a1 + a2) (Eigen Core/Redux.h; the tests hold this against the reference's own integrate / alloc code)
__device__ inline void xform(const float* T, float px, float py, float pz, float q[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = (T[4 * i] * px + (T[4 * i + 1] * py + T[4 * i + 2] * pz)) + T[4 * i + 3];
}
__device__ inline float robust_kernel(float val) { const float div = 1.0f + 2.0f * val; return 1.0f / (div * div * div); }   // math.cpp:43-47
__device__ inline bool within(const int* b, int x, int y, int z) { return !(x < b[0] || x > b[1] || y < b[2] || y > b[3] || z < b[4] || z > b[5]); }
// the clip test of SparseVoxelGrid::alloc (sparse_voxel_grid.cpp:439-445): the voxel's float world coordinates against {x0,x1,y0,y1,z0,z1}, faces inclusive.  ONE
// definition for the allocation of a frame, of a merge, and for the box criterion of i3d_fusion_prune
__device__ inline bool outside_box(const float* b, int x, int y, int z, float voxel_size) {
    const float wx = (float)x * voxel_size, wy = (float)y * voxel_size, wz = (float)z * voxel_size;
    return wx < b[0] || wx > b[1] || wy < b[2] || wy > b[3] || wz < b[4] || wz > b[5];
}

__global__ void k_clear(FusionTable t) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (i > t.mask) return;
    t.keys[i] = FUSION_EMPTY; t.sdf[i] = 0.0f; t.weight[i] = 0.0f; t.color[i] = make_uchar4(0, 0, 0, 0); t.rank[i] = ~0ull; t.crank[i] = ~0ull;
}
__global__ void k_rehash(FusionTable src, FusionTable dst) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (i > src.mask) return;
    const unsigned long long key = src.keys[i];
    if (key == FUSION_EMPTY) return;
    unsigned long long s = slot_of(key, dst.mask);
    for (;;) {
        if (atomicCAS(&dst.keys[s], FUSION_EMPTY, key) == FUSION_EMPTY) break;       // keys are unique in src
        s = (s + 1) & dst.mask;
    }
    dst.sdf[s] = src.sdf[i]; dst.weight[s] = src.weight[i]; dst.color[s] = src.color[i]; dst.rank[s] = src.rank[i]; dst.crank[s] = src.crank[i];
}

__global__ void k_erode(int w, int h, const float* __restrict__ in, int window, float max_diff, float* __restrict__ out) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= w || y >= h) return;
    const float d_ref = in[(size_t)y * w + x];
    bool valid = d_ref != 0.0f;
    if (valid && window > 0)
        for (int v = max(0, y - window); v <= min(y + window, h - 1); ++v)
            for (int u = max(0, x - window); u <= min(x + window, w - 1); ++u) {
                const float d = in[(size_t)v * w + u];
                if (d == 0.0f || fabsf(d - d_ref) > max_diff) valid = false;
            }
    out[(size_t)y * w + x] = valid ? d_ref : 0.0f;
}
__device__ inline void vertex(const FusionCam& c, const float* depth, int x, int y, float fx_inv, float fy_inv, float v[3]) {
    const float d = depth[(size_t)y * c.w + x];
    const float x0 = ((float)x - c.cx) * fx_inv, y0 = ((float)y - c.cy) * fy_inv;
    v[0] = x0 * d; v[1] = y0 * d; v[2] = d;
}
__global__ void k_normals(FusionCam c, const float* __restrict__ depth, float thr, float* __restrict__ normals) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= c.w || y >= c.h) return;
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (x >= 1 && y >= 1 && x < c.w - 1 && y < c.h - 1) {
        const float fx_inv = 1.0f / c.fx, fy_inv = 1.0f / c.fy;
        float v[3], x0[3], x1[3], y0[3], y1[3];
        vertex(c, depth, x, y, fx_inv, fy_inv, v); vertex(c, depth, x - 1, y, fx_inv, fy_inv, x0); vertex(c, depth, x + 1, y, fx_inv, fy_inv, x1);
        vertex(c, depth, x, y - 1, fx_inv, fy_inv, y0); vertex(c, depth, x, y + 1, fx_inv, fy_inv, y1);
        if (v[2] != 0.0f && x0[2] != 0.0f && x1[2] != 0.0f && y0[2] != 0.0f && y1[2] != 0.0f) {
            const float tx[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]}, ty[3] = {y1[0] - y0[0], y1[1] - y0[1], y1[2] - y0[2]};
            const float ntx = sqrtf(tx[0] * tx[0] + (tx[1] * tx[1] + tx[2] * tx[2])), nty = sqrtf(ty[0] * ty[0] + (ty[1] * ty[1] + ty[2] * ty[2]));
            if (ntx < thr && nty < thr) {
                n[0] = ty[1] * tx[2] - ty[2] * tx[1]; n[1] = ty[2] * tx[0] - ty[0] * tx[2]; n[2] = ty[0] * tx[1] - ty[1] * tx[0];
                const float sq = n[0] * n[0] + (n[1] * n[1] + n[2] * n[2]);
                if (sq > 0.0f) { const float l = sqrtf(sq); n[0] /= l; n[1] /= l; n[2] /= l; }
            }
        }
    }
    float* o = &normals[((size_t)y * c.w + x) * 3]; o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
}

// Allocation (SparseVoxelGrid::alloc) in two launches per frame.
// The reference walks every depth pixel's ray through the truncation band and inserts the 3x3x3 block around every voxel the ray enters —
// 27 map probes per ray sample, ~3.4e8 per VGA frame, nearly all of them finding the voxel present.  Here
//   1. k_alloc_centres (one lane per pixel) only records the CENTRE voxels: it makes sure the centre exists and keeps, per centre, the rank
//      of its first visit in the reference's sequential order (frame, pixel, ray step) with atomicMin — one probe per ray sample;
//   2. k_alloc_blocks (one lane per table slot) expands the block of every centre that has not been expanded in an earlier frame.
// A cell is first inserted by the earliest visit whose block covers it, and for one centre the earliest visit is its first, so the
// insertion rank of a new cell is  min over the centres c around it of (first visit of c, index of the cell in c's block)  — exactly
// what the atomicMin over the expanding centres computes.  A centre expanded once never needs expanding again (its cells exist):
// crank = 0 marks it, ~0 = never a centre, anything else = pending first-visit rank (i3d_fusion_prune, which may take cells away, sets every survivor back to
// ~0: section 38.1 item 5).  Both launches are idempotent, so a frame whose
// allocation ran out of table space is simply repeated after growth (the blocks launch does nothing when the centres launch overflowed).
// `fresh` counts the cells this lane created; the lanes of a wave add their totals to the global counter with ONE atomic at the end of
// the kernel (a same-address atomic per new voxel — ~1e6 per frame — serialises at ~10 ns each and was 3/4 of the allocation time).
__device__ inline bool insert_cell(const FusionTable& t, unsigned long long key, unsigned long long my_rank, unsigned long long limit, const unsigned long long* count,
                                   unsigned& fresh, int* overflow, unsigned long long* slot_out) {
    unsigned long long sl = slot_of(key, t.mask);
    for (unsigned long long probes = 0; probes <= t.mask; ++probes) {
        unsigned long long k = t.keys[sl];
        if (k == FUSION_EMPTY) {
            if (*count + fresh >= limit) break;                                   // the counter lags by what the waves in flight have not yet added: the
            k = atomicCAS(&t.keys[sl], FUSION_EMPTY, key);                        // probe bound above keeps a table that filled up meanwhile from spinning
            if (k == FUSION_EMPTY) { ++fresh; k = key; }
        }
        if (k == key) { if (my_rank < t.rank[sl]) atomicMin(&t.rank[sl], my_rank); *slot_out = sl; return true; }
        sl = (sl + 1) & t.mask;
    }
    *overflow = 1;
    return false;
}
__device__ inline void add_fresh(unsigned fresh, unsigned long long* count) {     // every lane of the wave must call this
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) fresh += __shfl_down(fresh, off);
    if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(count, (unsigned long long)fresh);
}
__global__ void k_alloc_centres(FusionTable t, FusionFrame f, FusionCam cam, const float* __restrict__ depth, unsigned long long limit,
                                unsigned long long* count, int* overflow) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    unsigned fresh = 0;
    const float d = (x < cam.w && y < cam.h) ? depth[(size_t)y * cam.w + x] : 0.0f;
    if (d != 0.0f) {
        const float pcx = 1.0f * (((float)x - cam.cx) / cam.fx), pcy = 1.0f * (((float)y - cam.cy) / cam.fy), pcz = 1.0f;     // unproject2(x, y, 1)
        const float ray_step = f.voxel_size * 0.25f, inv_vs = 1.0f / f.voxel_size;
        const unsigned long long pixel = (unsigned long long)y * cam.w + x;
        int lx = 0, ly = 0, lz = 0; unsigned step = 0;
        for (float d_off = -f.truncation; d_off <= f.truncation; d_off += ray_step, ++step) {
            const float s = d + d_off;
            float pw[3]; xform(f.c2w, pcx * s, pcy * s, pcz * s, pw);
            const int gx = round_trunc(pw[0] * inv_vs), gy = round_trunc(pw[1] * inv_vs), gz = round_trunc(pw[2] * inv_vs);
            if (gx == lx && gy == ly && gz == lz) continue;
            lx = gx; ly = gy; lz = gz;
            if (!within(f.bounds, gx, gy, gz)) continue;
            if (f.use_clip && outside_box(f.clip, gx, gy, gz, f.voxel_size)) continue;
            const unsigned long long visit = (f.frame << 41) | (pixel << 13) | ((unsigned long long)(step & 0xFF) << 5);
            unsigned long long sl;
            if (!insert_cell(t, pack_key(gx, gy, gz), visit | 13ull, limit, count, fresh, overflow, &sl)) break;      // the centre is cell 13 of its own block
            const unsigned long long pending = visit | 31ull;                                                       // never 0, never a cell rank
            const unsigned long long c = t.crank[sl];
            if (c != 0ull && pending < c) atomicMin(&t.crank[sl], pending);
        }
    }
    add_fresh(fresh, count);
}
__global__ void k_alloc_blocks(FusionTable t, unsigned long long limit, unsigned long long* count, int* overflow) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    unsigned fresh = 0;
    // a centre may only be expanded once its first-visit rank is final: if k_alloc_centres ran out of space, some lanes stopped early and a
    // pending rank may not be the minimum yet — leave everything pending for the repeat after growth
    const unsigned long long c = (i <= t.mask && !*overflow) ? t.crank[i] : 0ull;
    if (c != 0ull && c != ~0ull) {
        int gx, gy, gz; unpack_key(t.keys[i], gx, gy, gz);
        const unsigned long long visit = c & ~31ull;
        int blk = 0; bool ok = true;
        for (int bz = -1; bz <= 1 && ok; ++bz) for (int by = -1; by <= 1 && ok; ++by) for (int bx = -1; bx <= 1 && ok; ++bx, ++blk) {
            unsigned long long sl;
            ok = insert_cell(t, pack_key(gx + bx, gy + by, gz + bz), visit | (unsigned long long)blk, limit, count, fresh, overflow, &sl);
        }
        if (ok) t.crank[i] = 0ull;
    }
    add_fresh(fresh, count);
}

// The contribution of one frame to one voxel (sparse_voxel_grid.cpp:315-395): the gates (frustum bounds, z >= 0, pixel in the image, eroded
// depth > 0, sdf > -truncation), the sample d - z, the weight wu and the colour sample if the colour pixel is inside the colour image.  It depends on the voxel's
// key alone, never on its state.  ONE definition: integration adds it, de-integration takes the same numbers out again (k_deintegrate / k_reintegrate), and the
// debug lookup reports it (k_debug_frame_samples).
struct FrameSample { float sample, wu; bool has_color; unsigned char r, g, b; };
__device__ inline bool frame_sample(const FusionFrame& f, const FusionCam& dc, const FusionCam& cc, const float* __restrict__ depth, const float* __restrict__ normals,
                                    const uint8_t* __restrict__ bgr, int gx, int gy, int gz, FrameSample& s) {
    if (!within(f.bounds, gx, gy, gz)) return false;
    float p[3]; xform(f.w2c, (float)gx * f.voxel_size, (float)gy * f.voxel_size, (float)gz * f.voxel_size, p);
    if (p[2] < 0.0f) return false;
    int px = round_trunc((p[0] * dc.fx) / p[2] + dc.cx), py = round_trunc((p[1] * dc.fy) / p[2] + dc.cy);
    if (px < 0 || py < 0 || px >= dc.w || py >= dc.h) return false;
    const float d = depth[(size_t)py * dc.w + px];
    if (d <= 0.0f) return false;
    const float sdf = d - p[2];
    if (sdf <= -f.truncation) return false;
    const float tsdf = sdf >= 0.0f ? fminf(f.truncation, sdf) : fmaxf(-f.truncation, sdf);
    float wu = 1.0f;
    if (f.weight_sample > 0.0f) {
        const float* n = &normals[((size_t)py * dc.w + px) * 3];
        const float sq = p[0] * p[0] + (p[1] * p[1] + p[2] * p[2]);
        float pn[3] = {p[0], p[1], p[2]};
        if (sq > 0.0f) { const float l = sqrtf(sq); pn[0] /= l; pn[1] /= l; pn[2] /= l; }
        float wn = 1.0f - fabsf(pn[0] * n[0] + (pn[1] * n[1] + pn[2] * n[2]));
        wn = fmaxf(fminf(wn, 1.0f), 0.0f);
        wn = fmaxf(f.weight_sample * robust_kernel(wn), 1.0f);
        const float wd = fmaxf(f.weight_sample * robust_kernel(2.0f * fabsf(tsdf) / f.truncation), 1.0f);
        const float dn = (d - f.depth_min) / (f.depth_max - f.depth_min);
        const float wz = fmaxf(f.weight_sample * (1.0f - dn), 1.0f);
        wu = fmaxf(((wn + wd) + wz) / 3.0f, 3.0f);
    }
    s.sample = sdf; s.wu = wu; s.has_color = false; s.r = s.g = s.b = 0;
    px = round_trunc((p[0] * cc.fx) / p[2] + cc.cx); py = round_trunc((p[1] * cc.fy) / p[2] + cc.cy);
    if (px >= 0 && py >= 0 && px < cc.w && py < cc.h) {
        const uint8_t* c = &bgr[((size_t)py * cc.w + px) * 3];
        s.has_color = true; s.r = c[2]; s.g = c[1]; s.b = c[0];
    }
    return true;
}
// the running weighted mean takes the sample in (integrate's update, colour truncated as the reference's cast) ...
__device__ inline void sample_add(const FrameSample& s, float& sdf, float& weight, uchar4& col) {
    const float w_old = weight, w_new = w_old + s.wu;
    sdf = (sdf * w_old + s.sample * s.wu) / w_new;
    if (s.has_color) {
        col.x = (unsigned char)(((float)col.x * w_old + (float)s.r * s.wu) / w_new);
        col.y = (unsigned char)(((float)col.y * w_old + (float)s.g * s.wu) / w_new);
        col.z = (unsigned char)(((float)col.z * w_old + (float)s.b * s.wu) / w_new);
    }
    weight = w_new;
}
// ... and gives it back.  Below half the smallest weight a frame can add the voxel is Voxel() again: a voxel that only this frame fed
// gives exactly 0.  The colour is rounded to nearest with a clamp: integrate truncates, so the inverse must neither bias downwards a second time nor convert a
// negative float.
__device__ inline unsigned char color_sub(unsigned char c, unsigned char smp, float w_old, float wu, float w_new) {
    return (unsigned char)fminf(fmaxf(((float)c * w_old - (float)smp * wu) / w_new + 0.5f, 0.0f), 255.0f);
}
__device__ inline void sample_sub(const FrameSample& s, float& sdf, float& weight, uchar4& col) {
    const float w_old = weight, w_new = w_old - s.wu;
    if (w_new < 0.5f) { sdf = 0.0f; weight = 0.0f; col = make_uchar4(0, 0, 0, 0); return; }
    sdf = (sdf * w_old - s.sample * s.wu) / w_new;
    if (s.has_color) {
        col.x = color_sub(col.x, s.r, w_old, s.wu, w_new);
        col.y = color_sub(col.y, s.g, w_old, s.wu, w_new);
        col.z = color_sub(col.z, s.b, w_old, s.wu, w_new);
    }
    weight = w_new;
}

// one lane per table slot: the running weighted mean of one frame (sparse_voxel_grid.cpp:315-395)
__global__ void k_integrate(FusionTable t, FusionFrame f, FusionCam dc, FusionCam cc, const float* __restrict__ depth, const float* __restrict__ normals,
                            const uint8_t* __restrict__ bgr) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (i > t.mask) return;
    const unsigned long long key = t.keys[i];
    if (key == FUSION_EMPTY) return;
    int gx, gy, gz; unpack_key(key, gx, gy, gz);
    FrameSample s;
    if (!frame_sample(f, dc, cc, depth, normals, bgr, gx, gy, gz, s)) return;
    float sdf = t.sdf[i], weight = t.weight[i]; uchar4 col = t.color[i];
    sample_add(s, sdf, weight, col);
    t.sdf[i] = sdf; if (s.has_color) t.color[i] = col; t.weight[i] = weight;
}
// one lane per table slot: one frame's contribution taken out again.  A voxel first inserted by a LATER frame passes this frame's gates as well (they do not look
// at the voxel), but the frame never fed it: bits 41.. of the first-insertion rank are the ordinal of the inserting frame, and allocation precedes integration
// within a frame, so frame b fed voxel v exactly when (rank[v] >> 41) <= b and b's gates pass.  Keys, rank, crank and the count are not touched.
__global__ void k_deintegrate(FusionTable t, FusionFrame f, FusionCam dc, FusionCam cc, const float* __restrict__ depth, const float* __restrict__ normals,
                              const uint8_t* __restrict__ bgr) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (i > t.mask) return;
    const unsigned long long key = t.keys[i];
    if (key == FUSION_EMPTY) return;
    if ((t.rank[i] >> 41) > f.frame) return;                       // f.frame: the ordinal of the frame being taken out
    int gx, gy, gz; unpack_key(key, gx, gy, gz);
    FrameSample s;
    if (!frame_sample(f, dc, cc, depth, normals, bgr, gx, gy, gz, s)) return;
    float sdf = t.sdf[i], weight = t.weight[i]; uchar4 col = t.color[i];
    sample_sub(s, sdf, weight, col);
    t.sdf[i] = sdf; t.color[i] = col; t.weight[i] = weight;
}
// one lane per table slot: the frame of ordinal `out.frame` taken out at its old pose, then put in at the new one (whose cells the allocation before this launch
// has made, with the new ordinal — so the first half skips them).  The voxel's state stays in registers between the halves: one read and one write of the table
// where k_deintegrate + k_integrate make two, and the same fp32 operations in the same order, hence the same bits.
__global__ void k_reintegrate(FusionTable t, FusionFrame out, FusionFrame in, FusionCam dc, FusionCam cc, const float* __restrict__ depth, const float* __restrict__ normals,
                              const uint8_t* __restrict__ bgr) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (i > t.mask) return;
    const unsigned long long key = t.keys[i];
    if (key == FUSION_EMPTY) return;
    int gx, gy, gz; unpack_key(key, gx, gy, gz);
    FrameSample so, si;
    const bool sub = (t.rank[i] >> 41) <= out.frame && frame_sample(out, dc, cc, depth, normals, bgr, gx, gy, gz, so);
    const bool add = frame_sample(in, dc, cc, depth, normals, bgr, gx, gy, gz, si);
    if (!sub && !add) return;
    float sdf = t.sdf[i], weight = t.weight[i]; uchar4 col = t.color[i];
    if (sub) sample_sub(so, sdf, weight, col);
    if (add) sample_add(si, sdf, weight, col);
    t.sdf[i] = sdf; t.color[i] = col; t.weight[i] = weight;
}
__device__ inline bool key_in_range(const int* k) {
    return k[0] > -FUSION_COORD_OFFSET && k[0] < FUSION_COORD_OFFSET && k[1] > -FUSION_COORD_OFFSET && k[1] < FUSION_COORD_OFFSET && k[2] > -FUSION_COORD_OFFSET &&
           k[2] < FUSION_COORD_OFFSET;
}

// ---- a whole volume as the sample ----------------------------------------------------------------------------------------------------
// What src contributes to the lattice point (gx, gy, gz) of dst under x_dst = R x_src + t: ONE definition for the allocation, the update and nothing else.
//   ALIGNED   the src voxel k - m as it is stored, if its weight is not 0
//   general   p = R^T (k vs - t) in fp64; the cell of cell_of_point there (8 corners stored with weight != 0, the rule of i3d_fusion_query_points); the trilinear
//             sdf, weight and colour with tri_weights / tri_sum, the colour rounded to nearest
// A point whose image lies outside src's box [lo, hi) leaves before any probe.  On the general path the home slots of the 8 corners are read together first: an
// EMPTY home slot means the corner is not stored (linear probing, nothing is ever deleted from a table: i3d_fusion_prune builds a fresh one, section 38) and the point leaves after one round trip instead of a chain of up to 8;
// where all 8 are there the probes of load_cell find their first line in cache.
template <bool ALIGNED>
__device__ inline bool merge_sample(const FusionTable& src, const FusionMerge& mg, int gx, int gy, int gz, FrameSample& s) {
    if constexpr (ALIGNED) {
        const int k[3] = {gx - mg.m[0], gy - mg.m[1], gz - mg.m[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) if (k[a] < mg.lo[a] || k[a] >= mg.hi[a]) return false;
        if (!key_in_range(k)) return false;
        const long long sl = find_slot(src, pack_key(k[0], k[1], k[2]));
        if (sl < 0) return false;
        const float w = src.weight[sl];
        if (w == 0.0f) return false;
        const uchar4 c = src.color[sl];
        s.sample = src.sdf[sl]; s.wu = w; s.has_color = true; s.r = c.x; s.g = c.y; s.b = c.z;
        return true;
    } else {
        const double vs = (double)mg.voxel_size;
        const double d[3] = {(double)gx * vs - mg.t[0], (double)gy * vs - mg.t[1], (double)gz * vs - mg.t[2]};
        double p[3]; int b[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = (mg.R[a] * d[0] + mg.R[3 + a] * d[1]) + mg.R[6 + a] * d[2];
            const double q = p[a] / vs;                                               // cell_of_point's q: the same quotient, the same floor
            if (!(q >= (double)mg.lo[a] && q < (double)mg.hi[a])) return false;       // also a NaN; lo / hi are within the packed range, so the int below is safe
            b[a] = (int)floor(q);
        }
        unsigned long long home[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) home[i] = src.keys[slot_of(pack_key(b[0] + (i & 1), b[1] + ((i >> 1) & 1), b[2] + (i >> 2)), src.mask)];
        bool absent = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) absent |= home[i] == FUSION_EMPTY;
        if (absent) return false;
        const FusionRenderGrid g{src, vs, nullptr, {0, 0, 0}, {0, 0, 0}};
        CellCache cc; cell_cache_reset(cc);
        if (!cell_of_point(g, cc, p)) return false;
        double w[8], wt[8], cr[8], cg[8], cb[8];
        tri_weights(cc.f, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uchar4 c = src.color[cc.c[i]];
            wt[i] = (double)src.weight[cc.c[i]]; cr[i] = (double)c.x; cg[i] = (double)c.y; cb[i] = (double)c.z;
        }
        s.sample = (float)field(cc); s.wu = (float)tri_sum(w, wt); s.has_color = true;
        s.r = (unsigned char)(tri_sum(w, cr) + 0.5); s.g = (unsigned char)(tri_sum(w, cg) + 0.5); s.b = (unsigned char)(tri_sum(w, cb) + 0.5);
        return true;
    }
}
__device__ inline void add_count(bool on, unsigned long long* count) {            // every lane of the wave must call this: one atomic per wave
    const unsigned long long n = (unsigned long long)__popcll(__ballot(on));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, n);
}
// one lane per slot of src with weight != 0: the lattice points of dst that can take a sample because of it are made to exist.  General path: the 8 points
// floor(a) + {0,1}^3 around its image a = R k + t / vs — a lattice point with a valid sample lies in a src cell whose nearest corner is at most 1/2 away on every
// axis, hence less than sqrt(3)/2 < 1 away after the rotation on every axis, and that corner is stored with weight != 0 (section 27.1).  Aligned path: the one
// point k + m.  A candidate already in dst is skipped; a new one is inserted with the provisional rank (ordinal << 41) | (2^41 - 1) — launch_fusion_merge_rank
// writes the final one — if the clip box admits it and merge_sample is defined there.  `fresh`, `limit` and `overflow` as k_alloc_centres; idempotent.
template <bool ALIGNED>
__global__ void __launch_bounds__(TPB) k_merge_alloc(FusionTable dst, FusionTable src, FusionMerge mg, unsigned long long limit, unsigned long long* count, int* overflow,
                                                     unsigned long long* counts) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    unsigned fresh = 0;
    const unsigned long long key = i <= src.mask ? src.keys[i] : FUSION_EMPTY;
    const bool on = key != FUSION_EMPTY && src.weight[i] != 0.0f;
    if (on) {
        int kx, ky, kz; unpack_key(key, kx, ky, kz);
        int base[3]; bool ok = true;
        if constexpr (ALIGNED) {
            base[0] = kx + mg.m[0]; base[1] = ky + mg.m[1]; base[2] = kz + mg.m[2];
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double v = ((mg.R[3 * a] * (double)kx + mg.R[3 * a + 1] * (double)ky) + mg.R[3 * a + 2] * (double)kz) + mg.tv[a];
                ok &= fabs(v) < (double)FUSION_COORD_OFFSET;                          // also a NaN: the int conversion never sees such a value
                base[a] = ok ? (int)floor(v) : 0;
            }
        }
        const unsigned long long rank = (mg.ordinal << 41) | ((1ull << 41) - 1ull);
        for (int c = 0; ok && c < (ALIGNED ? 1 : 8); ++c) {
            const int k[3] = {base[0] + (c & 1), base[1] + ((c >> 1) & 1), base[2] + (c >> 2)};
            if (!key_in_range(k)) continue;
            const unsigned long long ck = pack_key(k[0], k[1], k[2]);
            if (find_slot(dst, ck) >= 0) continue;
            if (mg.use_clip && outside_box(mg.clip, k[0], k[1], k[2], mg.voxel_size)) continue;
            FrameSample s;
            if (!merge_sample<ALIGNED>(src, mg, k[0], k[1], k[2], s)) continue;
            unsigned long long sl;
            ok = insert_cell(dst, ck, rank, limit, count, fresh, overflow, &sl);
        }
    }
    add_fresh(fresh, count);
    add_count(on, &counts[0]);
}
// the voxels this merge inserted, listed in ascending packed key by slot_list.hip's SlotInserted: slot_sorted[j] gets the rank (ordinal << 41) | j - a function
// of the set of inserted keys, not of table slots
__global__ void k_merge_rank(FusionTable t, unsigned long long ordinal, long long n, const unsigned int* slot_sorted) {
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= n) return;
    t.rank[slot_sorted[j]] = (ordinal << 41) | (unsigned long long)j;
}
// one lane per slot of dst: src's sample at the voxel, if defined, enters it as a frame's sample does (sample_add).  No LDS, no atomics but the count's one per wave.
template <bool ALIGNED>
__global__ void __launch_bounds__(TPB) k_merge(FusionTable dst, FusionTable src, FusionMerge mg, unsigned long long* counts) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    const unsigned long long key = i <= dst.mask ? dst.keys[i] : FUSION_EMPTY;
    bool on = false;
    if (key != FUSION_EMPTY) {
        int gx, gy, gz; unpack_key(key, gx, gy, gz);
        FrameSample s;
        on = merge_sample<ALIGNED>(src, mg, gx, gy, gz, s);
        if (on) {
            float sdf = dst.sdf[i], weight = dst.weight[i]; uchar4 col = dst.color[i];
            sample_add(s, sdf, weight, col);
            dst.sdf[i] = sdf; dst.color[i] = col; dst.weight[i] = weight;
        }
    }
    add_count(on, &counts[1]);
}

// ---- records into an empty table: SparseVoxelGrid::load's loop data_[key] = voxel, one lane per record --------------------------------------
// The lane packs its key, probes from the key's home slot and claims the first empty slot with the 64-bit atomicCAS of insert_cell.  The winner of a slot is the
// only lane that ever writes the slot's values, so sdf, weight, colour (w = 0) and the rank i are plain stores: nothing reads them before the kernel ends.  crank
// stays ~0 (never a block centre).  A lane that meets its own key - stored by another lane of this launch, the table was empty - sets flags[0]: a duplicate.  The
// host sizes the table before the launch, so the probe bound is never reached; a lane that does reach it sets flags[1].  The key a probe reads may be stale only as
// EMPTY (a slot never returns to EMPTY), and then the CAS returns the stored key.  One atomic per wave adds the winners to the count (add_count).
__global__ void __launch_bounds__(TPB) k_insert_records(FusionTable t, long long n, const int* __restrict__ keys, const float* __restrict__ sdf,
                                                        const float* __restrict__ weight, const uint8_t* __restrict__ rgb, unsigned long long* count, int* flags) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    bool won = false;
    if (i < n) {
        const unsigned long long key = pack_key(keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]);
        unsigned long long sl = slot_of(key, t.mask), probes = 0;
        for (; probes <= t.mask; ++probes) {
            unsigned long long k = t.keys[sl];
            if (k == FUSION_EMPTY) {
                k = atomicCAS(&t.keys[sl], FUSION_EMPTY, key);
                if (k == FUSION_EMPTY) { won = true; break; }
            }
            if (k == key) { flags[0] = 1; break; }
            sl = (sl + 1) & t.mask;
        }
        if (won) {
            t.sdf[sl] = sdf[i]; t.weight[sl] = weight[i]; t.color[sl] = make_uchar4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0);
            t.rank[sl] = (unsigned long long)i;                                       // (ordinal 0 << 41) | position in the file
        } else if (probes > t.mask) flags[1] = 1;
    }
    add_count(won, count);
}

// ---- stored voxels dropped by weight, distance or box ----------------------------------------------------------------------------------------
// The verdict of slot i, one definition for the count and for the move: bit 0 = fails W (!(w > min_weight)), bit 1 = fails S (|s| > max_abs_sdf), bit 2 = fails B
// (outside the box in mode 1, inside it in mode 2), each only where the criterion is enabled; 0 for an EMPTY slot, whose key goes back through `key`.  The three
// loads of the slot do not depend on one another and are requested together, before the first of them is looked at (section 4.13): the barrier keeps the
// compiler from moving the weight and the sdf behind the test of the key, a second round trip for every stored slot.  They come back through `w` and `s`.
__device__ inline unsigned prune_verdict(const FusionTable& t, unsigned long long i, const FusionPrune& p, unsigned long long& key, float& w, float& s) {
    key = t.keys[i]; w = t.weight[i]; s = t.sdf[i];
    __builtin_amdgcn_sched_barrier(0);
    if (key == FUSION_EMPTY) return 0u;
    unsigned v = prune_fails_ws(p, w, s);
    if (p.box_mode != 0) {
        int x, y, z; unpack_key(key, x, y, z);
        if (outside_box(p.box, x, y, z, p.voxel_size) == (p.box_mode == 1)) v |= 4u;
    }
    return v;
}
// one lane per slot: counts = {stored, removed, failed W, failed S, failed B}, zeroed by the caller; one atomic per wave and counter (add_count).  Nothing is written
// to the table: the host reads the five numbers and decides whether anything moves at all.
__global__ void __launch_bounds__(TPB) k_prune_count(FusionTable t, FusionPrune p, unsigned long long* counts) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    unsigned long long key = FUSION_EMPTY; float w = 0.0f, s = 0.0f;
    const unsigned v = i <= t.mask ? prune_verdict(t, i, p, key, w, s) : 0u;
    add_count(key != FUSION_EMPTY, &counts[0]);
    add_count(v != 0u, &counts[1]);
    add_count((v & 1u) != 0u, &counts[2]);
    add_count((v & 2u) != 0u, &counts[3]);
    add_count((v & 4u) != 0u, &counts[4]);
}
// k_rehash with the verdict in front: one lane per slot of src, a survivor claims the first empty slot of the cleared table dst from its home slot on (keys are
// unique in src, and the host sized dst for the survivors, so the probe ends).  The winner of a slot is its only writer: plain stores behind the 64-bit CAS.  Key,
// values, all four bytes of the colour and the rank move as they are; crank becomes ~0, "never a centre": what crank == 0 promised - the 27 cells exist - is no
// longer known once a neighbour may have left (section 38.1 item 5).  The verdict is prune_verdict's, or, where `remove` is given (a launch argument: the branch is
// uniform), also the caller's byte for the slot: the components of section 39 decide by list entry, not by slot, and hand their decision over that way.
__global__ void __launch_bounds__(TPB) k_prune_rehash(FusionTable src, FusionTable dst, FusionPrune p, const unsigned char* __restrict__ remove) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (i > src.mask) return;
    unsigned long long key; float weight, sdf;
    const unsigned v = prune_verdict(src, i, p, key, weight, sdf);
    if (key == FUSION_EMPTY || v != 0u) return;
    if (remove && remove[i]) return;
    const uchar4 col = src.color[i]; const unsigned long long rank = src.rank[i];
    unsigned long long s = slot_of(key, dst.mask);
    for (unsigned long long probes = 0; probes <= dst.mask; ++probes) {
        if (atomicCAS(&dst.keys[s], FUSION_EMPTY, key) == FUSION_EMPTY) {
            dst.sdf[s] = sdf; dst.weight[s] = weight; dst.color[s] = col; dst.rank[s] = rank; dst.crank[s] = ~0ull;
            return;
        }
        s = (s + 1) & dst.mask;
    }
}

// tests only, by key lookup: the live table's state, and a frame's contribution (frame_sample) with no table involved
__global__ void k_debug_voxels(FusionTable t, long long n, const int* __restrict__ keys, uint8_t* found, float* sdf, float* weight, uint8_t* rgb, long long* first_frame) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int* k = &keys[3 * i];
    const long long s = key_in_range(k) ? find_slot(t, pack_key(k[0], k[1], k[2])) : -1;
    found[i] = s >= 0;
    sdf[i] = s >= 0 ? t.sdf[s] : 0.0f; weight[i] = s >= 0 ? t.weight[s] : 0.0f;
    const uchar4 c = s >= 0 ? t.color[s] : make_uchar4(0, 0, 0, 0);
    rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
    first_frame[i] = s >= 0 ? (long long)(t.rank[s] >> 41) : -1;
}
// tests only: the stored voxels at the (distinct) keys overwritten; a key that is not stored is reported and nothing is inserted
__global__ void k_debug_poke_voxels(FusionTable t, long long n, const int* __restrict__ keys, const float* __restrict__ sdf, const float* __restrict__ weight,
                                    const uint8_t* __restrict__ rgb, uint8_t* found) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int* k = &keys[3 * i];
    const long long s = key_in_range(k) ? find_slot(t, pack_key(k[0], k[1], k[2])) : -1;
    found[i] = s >= 0;
    if (s < 0) return;
    t.sdf[s] = sdf[i]; t.weight[s] = weight[i];
    uchar4 c = t.color[s]; c.x = rgb[3 * i]; c.y = rgb[3 * i + 1]; c.z = rgb[3 * i + 2];
    t.color[s] = c;
}
__global__ void k_debug_frame_samples(FusionFrame f, FusionCam dc, FusionCam cc, const float* __restrict__ depth, const float* __restrict__ normals,
                                      const uint8_t* __restrict__ bgr, long long n, const int* __restrict__ keys, uint8_t* on, float* sample, float* wu, uint8_t* has_color,
                                      uint8_t* rgb) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const int* k = &keys[3 * i];
    FrameSample s; s.sample = 0.0f; s.wu = 0.0f; s.has_color = false; s.r = s.g = s.b = 0;
    const bool ok = key_in_range(k) && frame_sample(f, dc, cc, depth, normals, bgr, k[0], k[1], k[2], s);
    on[i] = ok; sample[i] = ok ? s.sample : 0.0f; wu[i] = ok ? s.wu : 0.0f; has_color[i] = ok && s.has_color;
    rgb[3 * i] = s.r; rgb[3 * i + 1] = s.g; rgb[3 * i + 2] = s.b;
}

__global__ void k_keys(FusionTable t, long long m, const unsigned int* slot_sorted, int* kxyz) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    int x, y, z; unpack_key(t.keys[slot_sorted[i]], x, y, z);
    kxyz[3 * i] = x; kxyz[3 * i + 1] = y; kxyz[3 * i + 2] = z;
}
__global__ void k_positions(long long m, const unsigned int* slot_sorted, const int* order, unsigned int* visit_slot, int* pos_of_slot) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
    if (v >= m) return;
    const unsigned int s = slot_sorted[order[v]];
    visit_slot[v] = s; pos_of_slot[s] = (int)v;
}

// ---- correctSDF (sdf/algorithms.cpp:260-331) ----------------------------------------------------------------------------------
// The sweep is an in-place Gauss-Seidel pass in iteration order: voxel v sees the NEW value of neighbours visited before it and the
// OLD value of the others.  The sequential result is the unique fixed point of  cur[v] = F(v; cur[nb < v], old[nb > v]),  so k_correct is
// relaunched on `cur` until a launch changes nothing (voxel number k is final after at most k launches; in practice about ten).
// Hash probing 26 neighbours per voxel per launch costs 43 ms on 14M voxels (random 64-byte lines); instead the allocated voxels are
// sorted once by (brick, cell) so that spatial neighbours are neighbours in memory, the 26 neighbour indices are resolved once into a
// [26][m] table, and every launch is a coalesced read of that table plus short-range gathers.
__global__ void k_spatial_keys(FusionTable t, long long m, const unsigned int* slots, unsigned long long* skey) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const unsigned long long k = t.keys[slots[i]];
    const unsigned long long x = k & 0x1FFFFFull, y = (k >> 21) & 0x1FFFFFull, z = (k >> 42) & 0x1FFFFFull;
    skey[i] = ((z >> 3) << 45) | ((y >> 3) << 27) | ((x >> 3) << 9) | ((z & 7) << 6) | ((y & 7) << 3) | (x & 7);
}
__global__ void k_compact_init(FusionTable t, long long m, const unsigned int* slot_c, const int* pos_of_slot, int* compact_of_slot, float* c_sdf, int* c_pos,
                               unsigned char* c_valid, unsigned char* c_touched) {
    const long long c = (long long)blockIdx.x * TPB + threadIdx.x;
    if (c >= m) return;
    const unsigned int s = slot_c[c];
    compact_of_slot[s] = (int)c; c_sdf[c] = t.sdf[s]; c_pos[c] = pos_of_slot[s]; c_valid[c] = t.weight[s] > 0.0f; c_touched[c] = 0;
}
__global__ void k_build_nbr(FusionTable t, long long m, const unsigned int* slot_c, const int* compact_of_slot, const unsigned char* c_valid, int* nbr) {
    const long long c = (long long)blockIdx.x * TPB + threadIdx.x;
    if (c >= m) return;
    int gx, gy, gz; unpack_key(t.keys[slot_c[c]], gx, gy, gz);
    int n = 0;
    for (int k = -1; k <= 1; ++k) for (int j = -1; j <= 1; ++j) for (int i = -1; i <= 1; ++i) {
        if (k == 0 && j == 0 && i == 0) continue;
        int out = -1;
        if (c_valid[c]) {
            const long long nb = find_slot(t, pack_key(gx + i, gy + j, gz + k));
            if (nb >= 0) { const int cn = compact_of_slot[nb]; if (c_valid[cn]) out = cn; }
        }
        nbr[(long long)n * m + c] = out; ++n;
    }
}
__global__ void k_correct(FusionTable t, long long m, float voxel_size, const unsigned int* __restrict__ slot_c, const int* __restrict__ nbr, const int* __restrict__ c_pos,
                          const unsigned char* __restrict__ c_valid, const float* __restrict__ c_sdf, float* c_cur, unsigned char* c_upd, int* changed) {
    const long long c = (long long)blockIdx.x * TPB + threadIdx.x;
    if (c >= m || !c_valid[c]) return;
    const int v = c_pos[c];
    int gx, gy, gz; unpack_key(t.keys[slot_c[c]], gx, gy, gz);
    const float cx = (float)gx * voxel_size, cy = (float)gy * voxel_size, cz = (float)gz * voxel_size;
    const float old_f = c_sdf[c];
    const double sdf = (double)old_f, sgn = sdf >= 0.0 ? 1.0 : -1.0;
    float res = old_f; bool updated = false; int n = 0;
    // the 26 neighbours in THREE batches of unconditional loads (a missing neighbour reads this voxel's own slots): table entries, their visit positions, then the value each one
    // contributes — current sweep for voxels visited earlier, previous sweep otherwise.  One neighbour at a time this was a chain of three dependent loads behind a condition, 78
    // round trips per voxel and sweep (tools/isa_drains.py).  The compare-and-keep-the-last loop below is unchanged.
    int nbv[26]; float val[26];
#pragma unroll
    for (int q = 0; q < 26; ++q) nbv[q] = nbr[(long long)q * m + c];
    {
        int pos[26];
#pragma unroll
        for (int q = 0; q < 26; ++q) pos[q] = c_pos[nbv[q] >= 0 ? nbv[q] : (int)c];
#pragma unroll
        for (int q = 0; q < 26; ++q) { const int e = nbv[q] >= 0 ? nbv[q] : (int)c; val[q] = (pos[q] < v ? (const float*)c_cur : c_sdf)[e]; }
    }
#pragma unroll
    for (int k = -1; k <= 1; ++k)
#pragma unroll
    for (int j = -1; j <= 1; ++j)
#pragma unroll
    for (int i = -1; i <= 1; ++i) {
        if (k == 0 && j == 0 && i == 0) continue;
        const int nb = nbv[n]; const float vnb = val[n]; ++n;
        if (nb < 0) continue;
        const double sdf_nb = (double)vnb, sgn_nb = sdf_nb >= 0.0 ? 1.0 : -1.0;
        const float dx = cx - (float)(gx + i) * voxel_size, dy = cy - (float)(gy + j) * voxel_size, dz = cz - (float)(gz + k) * voxel_size;
        const double dist_nb = sdf_nb + sgn_nb * (double)sqrtf(dx * dx + (dy * dy + dz * dz));
        if (fabs(dist_nb) < fabs(sdf) && sgn == sgn_nb) { res = (float)dist_nb; updated = true; }
    }
    c_upd[c] = updated ? 1 : 0;
    if (__float_as_uint(c_cur[c]) != __float_as_uint(res)) { c_cur[c] = res; *changed = 1; }
}
__global__ void k_commit(long long m, const unsigned char* c_valid, const float* c_cur, const unsigned char* c_upd, float* c_sdf, unsigned char* c_touched, int* has_update) {
    const long long c = (long long)blockIdx.x * TPB + threadIdx.x;
    if (c >= m || !c_valid[c]) return;
    if (c_upd[c]) { c_sdf[c] = c_cur[c]; c_touched[c] = 1; *has_update = 1; }
}
__global__ void k_write_back(FusionTable t, long long m, const unsigned int* slot_c, const float* c_sdf, const unsigned char* c_touched) {
    const long long c = (long long)blockIdx.x * TPB + threadIdx.x;
    if (c >= m || !c_touched[c]) return;
    const unsigned int s = slot_c[c];
    t.sdf[s] = c_sdf[c]; t.weight[s] = 1.0f;
}
__global__ void k_valid(FusionTable t, long long m, const unsigned int* visit_slot, int* flags) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
    if (v >= m) return;
    flags[v] = t.weight[visit_slot[v]] > 0.0f;
}
__global__ void k_export(FusionTable t, long long m, const unsigned int* visit_slot, const int* flags, const int* offs, int* kxyz, float* sdf, float* weight, uint8_t* rgb) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
    if (v >= m || !flags[v]) return;
    const unsigned int s = visit_slot[v]; const long long o = offs[v];
    int x, y, z; unpack_key(t.keys[s], x, y, z);
    kxyz[3 * o] = x; kxyz[3 * o + 1] = y; kxyz[3 * o + 2] = z;
    sdf[o] = t.sdf[s]; weight[o] = t.weight[s];
    const uchar4 c = t.color[s]; rgb[3 * o] = c.x; rgb[3 * o + 1] = c.y; rgb[3 * o + 2] = c.z;
}

inline unsigned blocks(unsigned long long n) { return (unsigned)((n + TPB - 1) / TPB); }
inline dim3 image_grid(int w, int h) { return dim3((w + 31) / 32, (h + 7) / 8); }

}  // namespace

void launch_fusion_clear(hipStream_t st, FusionTable t) { hipLaunchKernelGGL(k_clear, blocks(t.mask + 1), TPB, 0, st, t); }
void launch_fusion_rehash(hipStream_t st, FusionTable src, FusionTable dst) { hipLaunchKernelGGL(k_rehash, blocks(src.mask + 1), TPB, 0, st, src, dst); }
void launch_erode(hipStream_t st, int w, int h, const float* in, int window, float max_diff, float* out) {
    hipLaunchKernelGGL(k_erode, image_grid(w, h), TPB, 0, st, w, h, in, window, max_diff, out);
}
void launch_normals(hipStream_t st, FusionCam cam, const float* depth, float thr, float* normals) {
    hipLaunchKernelGGL(k_normals, image_grid(cam.w, cam.h), TPB, 0, st, cam, depth, thr, normals);
}
void launch_fusion_alloc(hipStream_t st, FusionTable t, FusionFrame f, FusionCam cam, const float* depth, unsigned long long limit, unsigned long long* count, int* overflow) {
    hipLaunchKernelGGL(k_alloc_centres, image_grid(cam.w, cam.h), TPB, 0, st, t, f, cam, depth, limit, count, overflow);
    hipLaunchKernelGGL(k_alloc_blocks, blocks(t.mask + 1), TPB, 0, st, t, limit, count, overflow);
}
void launch_fusion_integrate(hipStream_t st, FusionTable t, FusionFrame f, FusionCam dcam, FusionCam ccam, const float* depth, const float* normals, const uint8_t* bgr) {
    hipLaunchKernelGGL(k_integrate, blocks(t.mask + 1), TPB, 0, st, t, f, dcam, ccam, depth, normals, bgr);
}
void launch_fusion_deintegrate(hipStream_t st, FusionTable t, FusionFrame f, FusionCam dcam, FusionCam ccam, const float* depth, const float* normals, const uint8_t* bgr) {
    hipLaunchKernelGGL(k_deintegrate, blocks(t.mask + 1), TPB, 0, st, t, f, dcam, ccam, depth, normals, bgr);
}
void launch_fusion_reintegrate(hipStream_t st, FusionTable t, FusionFrame out, FusionFrame in, FusionCam dcam, FusionCam ccam, const float* depth, const float* normals,
                               const uint8_t* bgr) {
    hipLaunchKernelGGL(k_reintegrate, blocks(t.mask + 1), TPB, 0, st, t, out, in, dcam, ccam, depth, normals, bgr);
}
void launch_fusion_merge_alloc(hipStream_t st, FusionTable dst, FusionTable src, FusionMerge mg, bool aligned, unsigned long long limit, unsigned long long* count, int* overflow,
                               unsigned long long* counts) {
    if (aligned) hipLaunchKernelGGL(k_merge_alloc<true>, blocks(src.mask + 1), TPB, 0, st, dst, src, mg, limit, count, overflow, counts);
    else hipLaunchKernelGGL(k_merge_alloc<false>, blocks(src.mask + 1), TPB, 0, st, dst, src, mg, limit, count, overflow, counts);
}
void launch_fusion_merge_rank(hipStream_t st, FusionTable t, unsigned long long ordinal, long long n, const unsigned int* slot_sorted) {
    if (n > 0) hipLaunchKernelGGL(k_merge_rank, blocks(n), TPB, 0, st, t, ordinal, n, slot_sorted);
}
void launch_fusion_merge(hipStream_t st, FusionTable dst, FusionTable src, FusionMerge mg, bool aligned, unsigned long long* counts) {
    if (aligned) hipLaunchKernelGGL(k_merge<true>, blocks(dst.mask + 1), TPB, 0, st, dst, src, mg, counts);
    else hipLaunchKernelGGL(k_merge<false>, blocks(dst.mask + 1), TPB, 0, st, dst, src, mg, counts);
}
void launch_fusion_insert_records(hipStream_t st, FusionTable t, long long n, const int* keys, const float* sdf, const float* weight, const uint8_t* rgb,
                                  unsigned long long* count, int* flags) {
    if (n > 0) hipLaunchKernelGGL(k_insert_records, blocks(n), TPB, 0, st, t, n, keys, sdf, weight, rgb, count, flags);
}
void launch_fusion_prune_count(hipStream_t st, FusionTable t, FusionPrune p, unsigned long long* counts) {
    hipLaunchKernelGGL(k_prune_count, blocks(t.mask + 1), TPB, 0, st, t, p, counts);
}
void launch_fusion_prune_rehash(hipStream_t st, FusionTable src, FusionTable dst, FusionPrune p, const unsigned char* remove) {
    hipLaunchKernelGGL(k_prune_rehash, blocks(src.mask + 1), TPB, 0, st, src, dst, p, remove);
}
void launch_fusion_debug_voxels(hipStream_t st, FusionTable t, long long n, const int* keys, uint8_t* found, float* sdf, float* weight, uint8_t* rgb, long long* first_frame) {
    if (n > 0) hipLaunchKernelGGL(k_debug_voxels, blocks(n), TPB, 0, st, t, n, keys, found, sdf, weight, rgb, first_frame);
}
void launch_fusion_debug_poke_voxels(hipStream_t st, FusionTable t, long long n, const int* keys, const float* sdf, const float* weight, const uint8_t* rgb, uint8_t* found) {
    if (n > 0) hipLaunchKernelGGL(k_debug_poke_voxels, blocks(n), TPB, 0, st, t, n, keys, sdf, weight, rgb, found);
}
void launch_fusion_debug_frame_samples(hipStream_t st, FusionFrame f, FusionCam dcam, FusionCam ccam, const float* depth, const float* normals, const uint8_t* bgr, long long n,
                                       const int* keys, uint8_t* on, float* sample, float* wu, uint8_t* has_color, uint8_t* rgb) {
    if (n > 0) hipLaunchKernelGGL(k_debug_frame_samples, blocks(n), TPB, 0, st, f, dcam, ccam, depth, normals, bgr, n, keys, on, sample, wu, has_color, rgb);
}
void launch_fusion_keys(hipStream_t st, FusionTable t, long long m, const unsigned int* slot_sorted, int* kxyz) {
    if (m > 0) hipLaunchKernelGGL(k_keys, blocks(m), TPB, 0, st, t, m, slot_sorted, kxyz);
}
void launch_fusion_positions(hipStream_t st, long long m, const unsigned int* slot_sorted, const int* order, unsigned int* visit_slot, int* pos_of_slot) {
    if (m > 0) hipLaunchKernelGGL(k_positions, blocks(m), TPB, 0, st, m, slot_sorted, order, visit_slot, pos_of_slot);
}
void launch_fusion_spatial_keys(hipStream_t st, FusionTable t, long long m, const unsigned int* slots, unsigned long long* skey) {
    if (m > 0) hipLaunchKernelGGL(k_spatial_keys, blocks(m), TPB, 0, st, t, m, slots, skey);
}
void launch_fusion_compact_init(hipStream_t st, FusionTable t, long long m, const unsigned int* slot_c, const int* pos_of_slot, int* compact_of_slot, float* c_sdf, int* c_pos,
                                unsigned char* c_valid, unsigned char* c_touched) {
    if (m > 0) hipLaunchKernelGGL(k_compact_init, blocks(m), TPB, 0, st, t, m, slot_c, pos_of_slot, compact_of_slot, c_sdf, c_pos, c_valid, c_touched);
}
void launch_fusion_build_nbr(hipStream_t st, FusionTable t, long long m, const unsigned int* slot_c, const int* compact_of_slot, const unsigned char* c_valid, int* nbr) {
    if (m > 0) hipLaunchKernelGGL(k_build_nbr, blocks(m), TPB, 0, st, t, m, slot_c, compact_of_slot, c_valid, nbr);
}
void launch_fusion_correct(hipStream_t st, FusionTable t, long long m, float voxel_size, const unsigned int* slot_c, const int* nbr, const int* c_pos, const unsigned char* c_valid,
                           const float* c_sdf, float* c_cur, unsigned char* c_upd, int* changed) {
    if (m > 0) hipLaunchKernelGGL(k_correct, blocks(m), TPB, 0, st, t, m, voxel_size, slot_c, nbr, c_pos, c_valid, c_sdf, c_cur, c_upd, changed);
}
void launch_fusion_commit(hipStream_t st, long long m, const unsigned char* c_valid, const float* c_cur, const unsigned char* c_upd, float* c_sdf, unsigned char* c_touched, int* has_update) {
    if (m > 0) hipLaunchKernelGGL(k_commit, blocks(m), TPB, 0, st, m, c_valid, c_cur, c_upd, c_sdf, c_touched, has_update);
}
void launch_fusion_write_back(hipStream_t st, FusionTable t, long long m, const unsigned int* slot_c, const float* c_sdf, const unsigned char* c_touched) {
    if (m > 0) hipLaunchKernelGGL(k_write_back, blocks(m), TPB, 0, st, t, m, slot_c, c_sdf, c_touched);
}
void launch_fusion_valid(hipStream_t st, FusionTable t, long long m, const unsigned int* visit_slot, int* flags) {
    if (m > 0) hipLaunchKernelGGL(k_valid, blocks(m), TPB, 0, st, t, m, visit_slot, flags);
}
void launch_fusion_export(hipStream_t st, FusionTable t, long long m, const unsigned int* visit_slot, const int* flags, const int* offsets, int* kxyz, float* sdf, float* weight, uint8_t* rgb) {
    if (m > 0) hipLaunchKernelGGL(k_export, blocks(m), TPB, 0, st, t, m, visit_slot, flags, offsets, kxyz, sdf, weight, rgb);
}

}  // namespace i3d
