// Alignment of one fusion volume to another on the stored fields (i3d_fusion_register_volume; the definition is DESIGN.md section 28).
//   k_register_volume_mean  the pivot pass and k_register_volume the pass of register_pass_device.hpp over the sorted list of src's selected voxels (slot_list.hpp's
//                           band selector): the point read from the list - 12 bytes of (key, sdf) instead of three doubles -, every entry counts towards the pivot,
//                           the corner prefilter below, and the residual r = f(R p + t) - s against the value src stores there.  s is constant in the pose: the
//                           Jacobian is k_register's
// The rows are totalled and the 6x6 step taken by k_track_solve (track_kernels.hip).  No floating-point atomics: every sum has an order that depends on the list
// alone, and the list on src's content alone (ascending packed key).
// Compiled with -ffp-contract=off: the numpy statement of the definition (tests/register_volume_twin.py) evaluates the same fp64 expressions in the same order.
#include "register_volume_kernels.hpp"
#include "register_pass_device.hpp"
#include "fusion_hash.hpp"

namespace i3d {
namespace {

using namespace fusion_hash;          // pack_key, unpack_key, slot_of (fusion_hash.hpp)

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

// list entries: the point of an entry is p[a] = (double)k[a] * vs, the residual the field minus the value src stores there
struct ListPoints {
    VolumeList list;
    __device__ void point(long long i, double (&p)[3]) const {
        int kx, ky, kz; unpack_key(list.keys[i], kx, ky, kz);
        p[0] = (double)kx * list.vs; p[1] = (double)ky * list.vs; p[2] = (double)kz * list.vs;
    }
    __device__ bool counts(const double (&)[3]) const { return true; }
    __device__ bool skip(const FusionRenderGrid& g, const double (&x)[3]) const { return corner_missing(g, x); }
    __device__ double residual(double f, long long i) const { return f - (double)list.sdf[i]; }
};

__global__ void __launch_bounds__(REGISTER_BLOCK) k_register_volume_mean(MeanParams prm, VolumeList list, double* __restrict__ slab) {
    register_mean_body(prm, ListPoints{list}, slab);
}

__global__ void __launch_bounds__(REGISTER_BLOCK) k_register_volume(FusionRenderGrid g, RegisterParams prm, VolumeList list, const TrackState* __restrict__ st,
                                                                    int check_done, double* __restrict__ slab) {
    register_pass_body(g, prm, ListPoints{list}, st, check_done, slab);
}

}  // namespace

void launch_register_volume_mean(hipStream_t st, const VolumeList& list, int per_lane, const double* R0, const double* t0, double vs_f, double* slab) {
    const int rows = register_rows(list.n, per_lane);
    if (rows > 0) k_register_volume_mean<<<rows, REGISTER_BLOCK, 0, st>>>(mean_params(list.n, per_lane, R0, t0, vs_f), list, slab);
}
void launch_register_volume(hipStream_t st, const FusionRenderGrid& g, const RegisterParams& p, const VolumeList& list, const TrackState* state, int check_done,
                            double* slab) {
    const int rows = register_rows(p.n, p.per_lane);
    if (rows > 0) k_register_volume<<<rows, REGISTER_BLOCK, 0, st>>>(g, p, list, state, check_done, slab);
}

}  // namespace i3d
