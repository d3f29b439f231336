// Rigid alignment of a point set to the stored field (i3d_register_points / i3d_fusion_register_points; the definition is DESIGN.md section 18).
//   k_register_mean  the pivot pass and k_register<G> the pass of register_pass_device.hpp over raw points: [n][3] doubles, a point counts towards the pivot with
//                    three finite coordinates, the residual is the field.  G = RenderGrid (the context's grid) or FusionRenderGrid (the fusion table as it stands)
// The rows are totalled and the 6x6 step taken by k_track_solve (track_kernels.hip).  No floating-point atomics: every sum has an order that depends on n alone.
// Compiled with -ffp-contract=off: the numpy statement of the definition (tests/register_twin.py) evaluates the same fp64 expressions in the same order.
#include "register_pass_device.hpp"

namespace i3d {
namespace {

// raw points: [n][3] doubles; the residual is the field itself
struct RawPoints {
    const double* __restrict__ points;
    __device__ void point(long long i, double (&p)[3]) const { p[0] = points[3 * i]; p[1] = points[3 * i + 1]; p[2] = points[3 * i + 2]; }
    __device__ bool counts(const double (&p)[3]) const { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }
    template <class G> __device__ bool skip(const G&, const double (&)[3]) const { return false; }
    __device__ double residual(double f, long long) const { return f; }
};

__global__ void __launch_bounds__(REGISTER_BLOCK) k_register_mean(MeanParams prm, const double* __restrict__ points, double* __restrict__ slab) {
    register_mean_body(prm, RawPoints{points}, slab);
}

template <class G>
__global__ void __launch_bounds__(REGISTER_BLOCK) k_register(G g, RegisterParams prm, const double* __restrict__ points, const TrackState* __restrict__ st,
                                                             int check_done, double* __restrict__ slab) {
    register_pass_body(g, prm, RawPoints{points}, st, check_done, slab);
}

template <class G>
void launch(hipStream_t st, const G& g, const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab) {
    const int rows = register_rows(p.n, p.per_lane);
    if (rows > 0) k_register<G><<<rows, REGISTER_BLOCK, 0, st>>>(g, p, points, state, check_done, slab);
}

}  // namespace

void launch_register_mean(hipStream_t st, long long n, int per_lane, const double* points, const double* R0, const double* t0, double vs, double* slab) {
    const int rows = register_rows(n, per_lane);
    if (rows > 0) k_register_mean<<<rows, REGISTER_BLOCK, 0, st>>>(mean_params(n, per_lane, R0, t0, vs), points, slab);
}
void launch_register(hipStream_t st, const RenderGrid& g, const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab) {
    launch(st, g, p, points, state, check_done, slab);
}
void launch_register(hipStream_t st, const FusionRenderGrid& g, const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab) {
    launch(st, g, p, points, state, check_done, slab);
}

}  // namespace i3d
