// Ray casting of the resident grid into one camera (render_kernels.hip, i3d_render_view).  The definition the kernel implements is DESIGN.md section 13; the same
// march over the fusion volume (i3d_fusion_render / i3d_fusion_track) is section 15.
#pragma once
#include "kernels.hpp"
#include "camera_device.hpp"
#include "fusion_kernels.hpp"

namespace i3d {

constexpr int RENDER_BRICK_SHIFT = 3;             // bricks of 8^3 voxels
constexpr int RENDER_MAX_SAMPLES = 1 << 14;       // safety bound of one ray's march (a ray across a 1000-voxel box with empty bricks skipped takes a few hundred)

struct RenderCam {                                // fp64 camera of the view, built on the host
    double R[9];                                  // world -> camera rotation, row-major
    double eye[3];                                // camera centre in the world frame (-R^T t)
    PinholeCam k;                                 // intrinsics, distortion and size of the view
    double tmin, tmax;                            // camera-z clip of the march (0 / +inf: open on that side)
};

struct RenderGrid {
    HashTable t; const int* nbr; int N;
    const float* weight; const double* sdf;       // sdf: x_sdf (sdf_refined) or sdf0 (fused)
    const double* alb; const float* sh;           // sh: [9][N]
    double vs;                                    // voxel size
    const unsigned* bits; int lo[3], dim[3];      // brick bitmap over the bricks' bounding box [lo, lo + dim), x fastest
    const uchar4* color;                          // the stored colour, x = R, y = G, z = B as k_permute / k_update_fields write it (the colour views alone); last: no other member moves
};

struct FusionRenderGrid {                         // the fusion volume as it stands: corners probed in the table, float sdf widened to fp64
    FusionTable t;
    double vs;                                    // voxel size
    const unsigned* bits; int lo[3], dim[3];      // brick bitmap over the table's slots with weight != 0, as RenderGrid's
};

struct RenderPlanes {                             // device planes, any may be null
    float* depth; float* normal /*[h][w][3]*/; float* albedo; float* shading; float* intensity; float* residual;
    const float* lum;                             // keyframe luminance of the level (residual only)
    int need_sh;                                  // shading / intensity / residual requested
};

struct RenderColorPlanes { float* depth; float* color /*[h][w][3] R,G,B*/; };      // the planes of a colour view, either may be null

struct RenderStatsDev { unsigned long long hits, samples; double residual_sq; };

// bounds[6] = {min x, y, z, max x, y, z} brick coordinates of the voxels with weight != 0 (the caller initialises them to INT_MAX / INT_MIN)
void launch_render_brick_bounds(hipStream_t st, int N, const int* cx, const int* cy, const int* cz, const float* weight, int* bounds);
// sets the bit of every brick that holds a voxel with weight != 0 (bits zeroed by the caller)
void launch_render_brick_fill(hipStream_t st, int N, const int* cx, const int* cy, const int* cz, const float* weight, unsigned* bits, const int lo[3], const int dim[3]);
void launch_render(hipStream_t st, const RenderGrid& g, const RenderCam& cam, const RenderPlanes& out, RenderStatsDev* stats);
// the same two steps over the slots of a fusion table (keys unpacked from the slot): bounds reduced per workgroup, then one atomic per workgroup and axis; the fill
// combines the lanes of a wave that set the same bitmap word into one atomicOr
void launch_fusion_brick_bounds(hipStream_t st, const FusionTable& t, int* bounds);
void launch_fusion_brick_fill(hipStream_t st, const FusionTable& t, unsigned* bits, const int lo[3], const int dim[3]);
// depth, world normal and the hit / sample stats only (out.albedo / shading / intensity / residual must be null)
void launch_render(hipStream_t st, const FusionRenderGrid& g, const RenderCam& cam, const RenderPlanes& out, RenderStatsDev* stats);
// the colour view (k_render<G, true>): the march of launch_render, then depth, the stored colour interpolated in the hit's cell and the stats, nothing else
void launch_render_color(hipStream_t st, const RenderGrid& g, const RenderCam& cam, const RenderColorPlanes& out, RenderStatsDev* stats);
void launch_render_color(hipStream_t st, const FusionRenderGrid& g, const RenderCam& cam, const RenderColorPlanes& out, RenderStatsDev* stats);

}  // namespace i3d
