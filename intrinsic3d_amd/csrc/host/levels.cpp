// Host side of the level transitions of Intrinsic3D::refine (refinement/intrinsic3d.cpp:206-409) around the device kernels of
// level_kernels.hip: recolourisation, thin-shell sparsification, x2 upsampling, the refine schedule itself, and the parity probe of the map order.
//
// Visit order (SURVEY.md hazard H1).  The reference keeps its voxels in std::unordered_map<Vec3i,...> (hash mat.h:117-124,
// reserve(64), max_load_factor 0.6: sparse_voxel_grid.cpp:52-53) and several results depend on that container's ITERATION order.
// Erasing keeps the relative order, so sparsification is a stable filter; upsampling and the initial Voxel -> VoxelSBR conversion
// build NEW maps, whose iteration order is a property of libstdc++'s container given the insertion sequence.  That order is
// obtained by replaying the container's list operations on the same key sequence (map_order.hpp; keys only, no voxel payload).
#include "context.hpp"
#include "../device/level_kernels.hpp"
#include <rocprim/rocprim.hpp>
#include "map_order.hpp"

namespace i3d {

// Intrinsic3D::recomputeColors (intrinsic3d.cpp:381-409): SDFColorization::add for every keyframe at pyramid level 0, then compute()
int recompute_colors(i3d_context* c, float occlusion_distance, int num_observations) {
    if (!c->have_grid || !c->have_frames || !c->have_camera) return ctx_fail(c, I3D_ERR_STATE, "recompute_colors: grid, keyframes and camera must be set");
    for (int f = 0; f < c->K; ++f) if (!c->bgr[(size_t)f * c->levels].p) return ctx_fail(c, I3D_ERR_STATE, "recompute_colors: keyframes were uploaded without colour images");
    if (num_observations > MAX_SLOTS || (num_observations <= 0 && c->K > MAX_SLOTS)) return ctx_fail(c, I3D_ERR_CAPACITY, "recompute_colors: more than 8 observations per voxel");
    OptParams p = camera_params(c, 0, occlusion_distance);
    std::vector<FrameConst> fc; build_frame_consts(c, 0, c->poses.data(), fc);
    CTX_HIP(c, ctx_upload(c, c->d_frames.p, fc.data(), fc.size()));
    { TimedScope t(c, I3D_K_OBSERVE); launch_recolor(c->stream, c->grid_view(), p, c->d_frames.p, num_observations, c->color.p); }
    CTX_HIP(c, ctx_sync(c));
    c->assembled = false;
    return I3D_OK;
}

// SDFAlgorithms::clearVoxelsOutsideThinShell (algorithms.cpp:368-458); erase keeps the iteration order of the survivors
int clear_outside_thin_shell(i3d_context* c, double thres_shell, int64_t* new_count) {
    if (!c->have_grid) return ctx_fail(c, I3D_ERR_STATE, "clear_outside_thin_shell: no grid");
    hipStream_t st = c->stream; const int N = c->N;
    GridView g = c->grid_view(); HashTable t{c->hkeys.p, c->hvals.p, c->hmask};
    DevBuf<int> keep, inv, keep_v, scan_v;
    CTX_HIP(c, keep.alloc(N)); CTX_HIP(c, keep_v.alloc(N)); CTX_HIP(c, scan_v.alloc(N));
    CTX_HIP(c, hipMemsetAsync(keep.p, 0, sizeof(int) * (size_t)N, st));
    launch_shell_mark(st, g, thres_shell, keep.p);
    launch_shell_crossing(st, g, t, keep.p);
    if (int rc = inverse_rank(c, inv)) return rc;
    launch_keep_visit(st, N, inv.p, keep.p, keep_v.p);
    CTX_HIP(c, rocprim::exclusive_scan(c->scan_tmp.p, c->scan_tmp_bytes, keep_v.p, scan_v.p, 0, (size_t)N, rocprim::plus<int>(), st));
    ScanTotal kept; CTX_HIP(c, kept.queue(c, keep_v.p, scan_v.p, N));
    CTX_HIP(c, ctx_sync(c));
    const int M = (int)kept.total();
    if (new_count) *new_count = M;
    if (M == N) return I3D_OK;
    if (M <= 0) return ctx_fail(c, I3D_ERR_STATE, "clear_outside_thin_shell: no voxel left");
    GridStaging s; CTX_HIP(c, s.alloc(M));
    launch_export_visit(st, g, inv.p, keep.p, scan_v.p, s.view());
    return set_grid_device(c, M, c->voxel_size, c->truncation, s);
}

// SDFAlgorithms::upsample (algorithms.cpp:202-235): the new grid has voxel_size/2 and truncation 5*voxel_size/2 (sparse_voxel_grid.cpp:44-49)
int upsample_grid(i3d_context* c, int64_t* new_count) {
    if (!c->have_grid) return ctx_fail(c, I3D_ERR_STATE, "upsample_grid: no grid");
    if ((long long)c->N * 8 > (1ll << 30)) return ctx_fail(c, I3D_ERR_CAPACITY, "upsample_grid: more than 2^30 voxels");
    hipStream_t st = c->stream; const int N = c->N; const long long M = 8ll * N;
    GridView g = c->grid_view(); HashTable t{c->hkeys.p, c->hvals.p, c->hmask};
    DevBuf<int> inv, perm; CTX_HIP(c, perm.alloc(M));
    GridStaging a, b; CTX_HIP(c, a.alloc(M)); CTX_HIP(c, b.alloc(M));
    if (int rc = inverse_rank(c, inv)) return rc;
    launch_upsample(st, g, t, inv.p, a.view());
    // iteration order of the new map, on the device (child keys are distinct: every parent has its own 2x2x2 block)
    { const std::vector<MapEpoch> ep = map_epochs((size_t)M);
      CTX_HIP(c, map_order_device(st, a.kxyz.p, (size_t)M, ep.data(), (int)ep.size(), perm.p)); }
    launch_permute_staging(st, M, perm.p, a.view(), b.view());
    CTX_HIP(c, ctx_sync(c));
    const float vs = c->voxel_size * 0.5f;
    if (new_count) *new_count = M;
    return set_grid_device(c, (int)M, vs, vs * 5.0f, b);
}

}  // namespace i3d

using namespace i3d;

extern "C" {

// parity probe: the replayed iteration order (mode 0: keys may repeat, 1: caller guarantees distinct keys) or the order of a real
// std::unordered_map (mode 2); returns the number of visited elements
int64_t i3d_debug_map_order(const int32_t* keys, int64_t n, int32_t mode, int32_t* order) {
    if (n < 0 || (n && (!keys || !order))) return -1;
    std::vector<int> o;
    if (mode == 2) map_iteration_order_stl(keys, (size_t)n, o);
    else if (mode == 3) map_iteration_order_epochs(keys, (size_t)n, o);
    else if (mode == 4) {                                     // the device path (distinct keys)
        if (n == 0) return 0;
        int *dk = nullptr, *dout = nullptr;
        const std::vector<MapEpoch> ep = map_epochs((size_t)n);
        bool ok = hipMalloc((void**)&dk, sizeof(int) * 3 * (size_t)n) == hipSuccess && hipMalloc((void**)&dout, sizeof(int) * (size_t)n) == hipSuccess
                  && hipMemcpy(dk, keys, sizeof(int) * 3 * (size_t)n, hipMemcpyHostToDevice) == hipSuccess
                  && map_order_device(nullptr, dk, (size_t)n, ep.data(), (int)ep.size(), dout) == hipSuccess
                  && hipMemcpy(order, dout, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
        if (dk) (void)hipFree(dk); if (dout) (void)hipFree(dout);
        return ok ? n : -1;
    }
    else map_iteration_order_replay(keys, (size_t)n, o, mode == 1);
    for (size_t i = 0; i < o.size(); ++i) order[i] = o[i];
    return (int64_t)o.size();
}
int i3d_recompute_colors(i3d_context* c, float occlusion_distance, int32_t num_observations) {
    CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT);
    return recompute_colors(c, occlusion_distance, num_observations);
}
int i3d_clear_outside_thin_shell(i3d_context* c, double thres_shell, int64_t* new_count) {
    CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT);
    return clear_outside_thin_shell(c, thres_shell, new_count);
}
int i3d_upsample(i3d_context* c, int64_t* new_count) {
    CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT);
    return upsample_grid(c, new_count);
}

// Intrinsic3D::refine (intrinsic3d.cpp:206-290) on the resident grid / keyframes / camera
int i3d_refine(i3d_context* c, const i3d_refine_config* rc, const i3d_optimizer_config* oc, i3d_refine_callback cb, void* user) {
    CTX_ENTER(c, rc && oc, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_refine: null argument"));
    if (!c->have_grid || rc->num_grid_levels <= 0 || rc->num_rgbd_levels <= 0) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_refine: no grid or no levels");   // :208-211
    if (rc->num_rgbd_levels > c->levels) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_refine: more rgbd levels than uploaded pyramid levels");
    int rcode = recompute_colors(c, rc->occlusion_distance, rc->num_observations);            // init(): initial SDF recolorization (:196-201)
    if (rcode) return rcode;
    const int coarsest = rc->num_grid_levels - 1;
    for (int gl = coarsest; gl >= 0; --gl) {
        double factor = rc->thin_shell_factor;                                                 // prepareGridLevel (:298-316)
        if (rc->thin_shell_factor_final > 0.0) factor = varying_lambda(coarsest - gl, rc->num_grid_levels, rc->thin_shell_factor, rc->thin_shell_factor_final);
        const double thres = factor * (double)c->voxel_size;
        if (rc->clear_distant_voxels) { rcode = clear_outside_thin_shell(c, thres, nullptr); if (rcode) return rcode; }
        for (int pl = rc->num_rgbd_levels - 1; pl >= 0; --pl) {
            if (pl > 0 && gl < coarsest) continue;                                             // all pyramid levels only on the coarsest grid (:245)
            i3d_sh_stats shst; int32_t S = 0;
            rcode = estimate_sh(c, rc->subvolume_size_sh, rc->sh_lambda_reg, thres, &S, nullptr, nullptr, 1 << 30, &shst);
            if (rcode) break;                                                                  // "lighting estimation not successful": leave the rgbd loop (:257-261)
            i3d_optimizer_config o = *oc; o.thres_shell = thres; o.grid_level = gl; o.rgbd_level = pl;
            o.occlusion_distance = rc->occlusion_distance; o.num_observations = rc->num_observations;
            rcode = optimize(c, o, nullptr);
            if (rcode && rcode != I3D_ERR_INVALID_ARGUMENT) return rcode;                      // the reference logs a failed optimize and goes on (:273-276)
            rcode = recompute_colors(c, rc->occlusion_distance, rc->num_observations);         // finishRgbdLevel (:353-378)
            if (rcode) return rcode;
            if (cb) cb(user, gl, rc->num_grid_levels, pl, rc->num_rgbd_levels);                // notifyCallbacks -> onSDFRefined (:282)
        }
        if (gl > 0) { rcode = upsample_grid(c, nullptr); if (rcode) return rcode; }            // finishGridLevel (:320-333)
    }
    return I3D_OK;
}

}  // extern "C"

