// Alignment of one fusion volume to another on the stored fields (i3d_fusion_register_volume; the definition is DESIGN.md section 28).
//   k_volume_select_flag / k_volume_select_gather   one lane per slot of src: the slots of section 28.1 item 2, and their (packed key, sdf) at the scanned offsets
//   k_register_volume_mean  the pivot: per workgroup the sum and the number of the list's points that count, one slab row
//   k_register_volume       k_register<FusionRenderGrid> (register_kernels.hip) with the point read from the list - 12 bytes of (key, sdf) instead of three
//                           doubles - and the residual r = f(R p + t) - s against the value src stores there.  s is constant in the pose: the Jacobian is k_register's
// The rows are totalled and the 6x6 step taken by k_track_solve (track_kernels.hip).  No floating-point atomics: every sum has an order that depends on the list
// alone, and the list on src's content alone (ascending packed key).
// Compiled with -ffp-contract=off: the numpy statement of the definition (tests/register_volume_twin.py) evaluates the same fp64 expressions in the same order.
#include "register_volume_kernels.hpp"
#include "point_cell_device.hpp"
#include "slab_device.hpp"

namespace i3d {
namespace {

using namespace fusion_hash;          // pack_key, unpack_key, slot_of (fusion_hash.hpp)

constexpr int SELECT_BLOCK = 256;

__device__ inline bool on_stride(int k, int stride) {          // floor modulus: -4 is on stride 2 and on stride 4, -3 on neither
    int m = k % stride;
    if (m < 0) m += stride;
    return m == 0;
}

__device__ inline bool selected(const FusionTable& src, const VolumeSelect& sel, unsigned long long i) {
    const unsigned long long key = src.keys[i];
    if (key == FUSION_EMPTY || src.weight[i] == 0.0f) return false;
    if (!(fabs((double)src.sdf[i]) <= sel.band)) return false;           // also a NaN
    int kx, ky, kz; unpack_key(key, kx, ky, kz);
    return on_stride(kx, sel.stride) && on_stride(ky, sel.stride) && on_stride(kz, sel.stride);
}

__global__ void __launch_bounds__(SELECT_BLOCK) k_volume_select_flag(FusionTable src, VolumeSelect sel, int* __restrict__ flags) {
    const unsigned long long i = (unsigned long long)blockIdx.x * SELECT_BLOCK + threadIdx.x;
    if (i > src.mask) return;
    flags[i] = selected(src, sel, i) ? 1 : 0;
}

__global__ void __launch_bounds__(SELECT_BLOCK) k_volume_select_gather(FusionTable src, const int* __restrict__ flags, const int* __restrict__ offs, long long n,
                                                                       unsigned long long* __restrict__ keys, float* __restrict__ sdf) {
    const unsigned long long i = (unsigned long long)blockIdx.x * SELECT_BLOCK + threadIdx.x;
    if (i > src.mask || !flags[i]) return;
    const long long at = offs[i];
    if (at < 0 || at >= n) return;                   // n = the scanned count: the buffers' size
    keys[at] = src.keys[i]; sdf[at] = src.sdf[i];
}

// the point of a list entry: p[a] = (double)k[a] * vs
__device__ inline void list_point(const VolumeList& list, long long i, double (&p)[3]) {
    int kx, ky, kz; unpack_key(list.keys[i], kx, ky, kz);
    p[0] = (double)kx * list.vs; p[1] = (double)ky * list.vs; p[2] = (double)kz * list.vs;
}

struct MeanParams { int per_lane; double R[9], t[3], vs; };

__global__ void __launch_bounds__(REGISTER_BLOCK) k_register_volume_mean(MeanParams prm, VolumeList list, double* __restrict__ slab) {
    __shared__ double part[REGISTER_BLOCK / 64][TRACK_COLS];
    double s[TRACK_COLS];
#pragma unroll
    for (int k = 0; k < TRACK_COLS; ++k) s[k] = 0.0;
    const long long base = (long long)blockIdx.x * REGISTER_BLOCK * prm.per_lane + threadIdx.x;
    for (int j = 0; j < prm.per_lane; ++j) {
        const long long i = base + (long long)j * REGISTER_BLOCK;
        if (i < list.n) {                            // tail lanes fall through to the shuffles with zeros
            double p[3]; list_point(list, i, p);
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double x = ((prm.R[3 * a] * p[0] + prm.R[3 * a + 1] * p[1]) + prm.R[3 * a + 2] * p[2]) + prm.t[a];
                ok = ok && isfinite(x) && fabs(x / prm.vs) < QUERY_MAX_COORD;
            }
            if (ok) { s[0] = s[0] + p[0]; s[1] = s[1] + p[1]; s[2] = s[2] + p[2]; s[3] = s[3] + 1.0; }
        }
    }
    slab_row(s, part, slab);
}

// The home slots of the 8 corners of the cell under x in f's table, read together before cell_of_point probes them one after another (merge_sample's device,
// DESIGN.md 27.2): an EMPTY home slot means that corner is not stored (linear probing, nothing is ever deleted), so the cell is not valid and the point leaves
// after one round trip; where all 8 are there the probes of load_cell find their first line in cache.  Decides nothing cell_of_point would decide otherwise.
__device__ inline bool corner_missing(const FusionRenderGrid& g, const double (&x)[3]) {
    int b[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double q = x[a] / g.vs;
        if (!isfinite(x[a]) || !(fabs(q) < QUERY_MAX_COORD)) return true;
        b[a] = (int)floor(q);
        if (b[a] < -FUSION_COORD_OFFSET || b[a] >= FUSION_COORD_OFFSET - 1) return true;      // load_cell's range: no packed key for a corner
    }
    unsigned long long home[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) home[i] = g.t.keys[slot_of(pack_key(b[0] + (i & 1), b[1] + ((i >> 1) & 1), b[2] + (i >> 2)), g.t.mask)];
    bool absent = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) absent |= home[i] == FUSION_EMPTY;
    return absent;
}

__global__ void __launch_bounds__(REGISTER_BLOCK) k_register_volume(FusionRenderGrid g, RegisterParams prm, VolumeList list, const TrackState* __restrict__ st,
                                                                    int check_done, double* __restrict__ slab) {
    __shared__ double part[REGISTER_BLOCK / 64][TRACK_COLS];
    if (check_done && st->done) return;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = st->R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = st->t[i];
    const double vs = g.vs;
    double s[TRACK_COLS];
#pragma unroll
    for (int k = 0; k < TRACK_COLS; ++k) s[k] = 0.0;
    const long long base = (long long)blockIdx.x * REGISTER_BLOCK * prm.per_lane + threadIdx.x;
    for (int j = 0; j < prm.per_lane; ++j) {
        const long long i = base + (long long)j * REGISTER_BLOCK;
        if (i >= prm.n) break;                       // tail lanes fall through to the shuffles with zeros
        double p[3]; list_point(list, i, p);
        const double stored = (double)list.sdf[i];
        double xp[3], x[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xp[a] = ((R[3 * a] * p[0] + R[3 * a + 1] * p[1]) + R[3 * a + 2] * p[2]) + t[a];
            x[a] = xp[a] + prm.c[a];
        }
        if (corner_missing(g, x)) continue;
        CellCache cc; cell_cache_reset(cc);
        if (!cell_of_point(g, cc, x)) continue;
        s[29] = s[29] + 1.0;
        const double r = field(cc) - stored;
        if (!(fabs(r) <= prm.max_distance)) continue;
        double gr[3]; cell_gradient(cc, gr);
        const double d0 = gr[0] / vs, d1 = gr[1] / vs, d2 = gr[2] / vs;
        const double J[6] = {xp[1] * d2 - xp[2] * d1, xp[2] * d0 - xp[0] * d2, xp[0] * d1 - xp[1] * d0, d0, d1, d2};
        add_normal_row(s, J, r, 27, [](double x) { return x; });
    }
    slab_row(s, part, slab);
}

unsigned select_blocks(const FusionTable& t) { return (unsigned)((t.mask + SELECT_BLOCK) / SELECT_BLOCK); }

}  // namespace

void launch_volume_select_flag(hipStream_t st, FusionTable src, VolumeSelect sel, int* flags) {
    k_volume_select_flag<<<select_blocks(src), SELECT_BLOCK, 0, st>>>(src, sel, flags);
}
void launch_volume_select_gather(hipStream_t st, FusionTable src, const int* flags, const int* offsets, long long n, unsigned long long* keys, float* sdf) {
    k_volume_select_gather<<<select_blocks(src), SELECT_BLOCK, 0, st>>>(src, flags, offsets, n, keys, sdf);
}
void launch_register_volume_mean(hipStream_t st, const VolumeList& list, int per_lane, const double* R0, const double* t0, double vs_f, double* slab) {
    MeanParams prm; prm.per_lane = per_lane; prm.vs = vs_f;
    for (int i = 0; i < 9; ++i) prm.R[i] = R0[i];
    for (int a = 0; a < 3; ++a) prm.t[a] = t0[a];
    const int rows = register_rows(list.n, per_lane);
    if (rows > 0) k_register_volume_mean<<<rows, REGISTER_BLOCK, 0, st>>>(prm, list, slab);
}
void launch_register_volume(hipStream_t st, const FusionRenderGrid& g, const RegisterParams& p, const VolumeList& list, const TrackState* state, int check_done,
                            double* slab) {
    const int rows = register_rows(p.n, p.per_lane);
    if (rows > 0) k_register_volume<<<rows, REGISTER_BLOCK, 0, st>>>(g, p, list, state, check_done, slab);
}

}  // namespace i3d
