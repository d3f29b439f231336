// The caller's own rays on the stored field (cast_rays_kernels.hip, i3d_cast_rays / i3d_fusion_cast_rays).  The definition is DESIGN.md section 34: the march
// of section 13 (ray_march_device.hpp) with a per-ray origin, direction and range.
#pragma once
#include "render_kernels.hpp"
#include "query_kernels.hpp"

namespace i3d {

constexpr int CAST_BLOCK = 256;                   // one lane per ray
constexpr int CAST_VALID = 1, CAST_HIT = 2, CAST_BUDGET = 4;      // the status bits

struct CastRays {                                 // device arrays of one call
    long long n;
    const double* origins; const double* directions;      // [n][3]
    const double* t_min; const double* t_max;             // [n], either may be null: 0 / +inf
    const unsigned* perm;                                 // lane j marches ray perm[j]; null: ray j
    double* t; double* position /*[n][3]*/; float* normal /*[n][3]*/; float* albedo; float* shading; float* intensity; unsigned char* status;     // any may be null
    int need_sh;                                          // shading / intensity requested
};

// the arrays of a colour call: the rays, perm, t and status of CastRays (its other outputs are not read) and the colour
struct CastRaysColor : CastRays { float* color /*[n][3] R,G,B*/; };

// what the key of a ray reads of the model: the voxel size and the bitmap's box
struct CastBox { double vs; int lo[3], dim[3]; };

// one lane per ray, every requested output written at the ray's own index; stats: hits and samples added (zeroed by the caller)
void launch_cast_rays(hipStream_t st, const RenderGrid& g, const CastRays& p, RenderStatsDev* stats);
// t, position, normal, status and the stats only (p.albedo / shading / intensity must be null)
void launch_cast_rays(hipStream_t st, const FusionRenderGrid& g, const CastRays& p, RenderStatsDev* stats);
// the colour call (k_cast_rays<G, true>): t, status, the stored colour interpolated in the hit's cell and the stats, nothing else
void launch_cast_rays_color(hipStream_t st, const RenderGrid& g, const CastRaysColor& p, RenderStatsDev* stats);
void launch_cast_rays_color(hipStream_t st, const FusionRenderGrid& g, const CastRaysColor& p, RenderStatsDev* stats);

// the coherent order.  coord_bits: the bits of a brick coordinate relative to box.lo (the smallest with 2^coord_bits >= every box.dim, >= 1);
// a key has cast_key_bits(coord_bits) of them: [miss | octant of the direction's signs : 3 | Morton code of the entry brick : 3 coord_bits]
inline int cast_coord_bits(const int dim[3]) { int b = 1; while (b < 20 && ((1 << b) < dim[0] || (1 << b) < dim[1] || (1 << b) < dim[2])) ++b; return b; }
inline int cast_key_bits(int coord_bits) { return 3 * coord_bits + 4; }
void launch_cast_ray_keys(hipStream_t st, const CastBox& box, const CastRays& p, int coord_bits, unsigned long long* keys, unsigned* index);
size_t cast_sort_temp_bytes(long long n, int key_bits);
hipError_t launch_cast_sort(hipStream_t st, void* temp, size_t temp_bytes, const unsigned long long* keys_in, unsigned long long* keys_out, const unsigned* index_in,
                            unsigned* index_out, long long n, int key_bits);

}  // namespace i3d
