// Grid in and out: the caller's arrays in visit order -> the resident grid in device order (set_grid, set_grid_from_tsdf_records, set_grid_device for the level
// transitions) and back (get_grid, update_grid, export_grid, grid_info), and the per-voxel SH pair.
#include "context.hpp"
#include "../device/level_kernels.hpp"
#include <rocprim/rocprim.hpp>
#include "map_order.hpp"

namespace i3d {
int set_grid_device(i3d_context* c, int N, float voxel_size, float truncation, GridStaging& g) {
    c->N = N; c->voxel_size = voxel_size; c->truncation = truncation; c->have_grid = false; c->have_sh = false; c->have_subvolumes = false; c->assembled = false;
    c->model.bricks.ok = false;       // the stored voxels change: the brick bitmap of the renderer is rebuilt on its next call
    c->slots = 0;      // row storage is sized by N: force a re-allocation for the new grid
    hipStream_t st = c->stream;
    DevBuf<int> perm, iota; DevBuf<unsigned long long> skeys, skeys2;
    CTX_HIP(c, perm.alloc(N)); CTX_HIP(c, iota.alloc(N)); CTX_HIP(c, skeys.alloc(N)); CTX_HIP(c, skeys2.alloc(N));
    // brick-Morton sort (device order), then permute every field into SoA planes
    launch_sort_keys(st, N, g.kxyz.p, skeys.p, iota.p);
    size_t tmp_bytes = 0;
    CTX_HIP(c, rocprim::radix_sort_pairs(nullptr, tmp_bytes, skeys.p, skeys2.p, iota.p, perm.p, (size_t)N, 0, 64, st));
    DevBuf<unsigned char> tmp; CTX_HIP(c, tmp.alloc(tmp_bytes));
    CTX_HIP(c, rocprim::radix_sort_pairs(tmp.p, tmp_bytes, skeys.p, skeys2.p, iota.p, perm.p, (size_t)N, 0, 64, st));
    // grid-sized buffers: release and re-allocate when the voxel count changes (level transitions shrink and grow the grid)
    auto fit = [&](auto& buf, size_t n) -> hipError_t { if (buf.n != n) buf.release(); return buf.alloc(n); };
    CTX_HIP(c, fit(c->cx, N)); CTX_HIP(c, fit(c->cy, N)); CTX_HIP(c, fit(c->cz, N)); CTX_HIP(c, fit(c->rank, N));
    CTX_HIP(c, fit(c->sdf0, N)); CTX_HIP(c, fit(c->x_sdf, N)); CTX_HIP(c, fit(c->x_alb, N)); CTX_HIP(c, fit(c->xc_sdf, N)); CTX_HIP(c, fit(c->xc_alb, N));
    CTX_HIP(c, fit(c->f_sdf, N)); CTX_HIP(c, fit(c->f_alb, N)); CTX_HIP(c, fit(c->weight, N)); CTX_HIP(c, fit(c->color, N));
    CTX_HIP(c, fit(c->flags, N)); CTX_HIP(c, fit(c->aidx, N)); CTX_HIP(c, fit(c->alist, N)); CTX_HIP(c, fit(c->aflag, N)); CTX_HIP(c, fit(c->ascan, N));
    CTX_HIP(c, fit(c->sh, (size_t)9 * N)); CTX_HIP(c, fit(c->nbr, (size_t)NUM_NBR * N));
    launch_permute_grid(st, N, perm.p, g.view(), c->cx.p, c->cy.p, c->cz.p, c->rank.p, c->sdf0.p,
                        c->x_sdf.p, c->x_alb.p, c->f_sdf.p, c->f_alb.p, c->weight.p, c->color.p);
    CTX_HIP(c, hipMemcpyAsync(c->xc_sdf.p, c->x_sdf.p, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, st));
    CTX_HIP(c, hipMemcpyAsync(c->xc_alb.p, c->x_alb.p, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, st));
    // device hash (2x load-factor headroom, power of two) + neighbour table; the hash stays resident for the level kernels
    unsigned int cap = 1; while (cap < (unsigned int)N * 2u) cap <<= 1;
    CTX_HIP(c, fit(c->hkeys, cap)); CTX_HIP(c, fit(c->hvals, cap)); c->hmask = cap - 1;
    CTX_HIP(c, hipMemsetAsync(c->hkeys.p, 0xff, sizeof(unsigned long long) * (size_t)cap, st));
    HashTable t{c->hkeys.p, c->hvals.p, cap - 1};
    launch_hash_build(st, N, c->cx.p, c->cy.p, c->cz.p, t);
    launch_nbr_build(st, N, c->cx.p, c->cy.p, c->cz.p, t, c->nbr.p);
    CTX_HIP(c, hipMemsetAsync(c->sh.p, 0, sizeof(float) * 9 * (size_t)N, st));
    size_t sb = 0;
    CTX_HIP(c, rocprim::exclusive_scan(nullptr, sb, c->aflag.p, c->ascan.p, 0, (size_t)N, rocprim::plus<int>(), st));
    c->scan_tmp.release(); CTX_HIP(c, c->scan_tmp.alloc(sb ? sb : 1)); c->scan_tmp_bytes = sb;
    CTX_HIP(c, hipStreamSynchronize(st));
    CTX_HIP(c, hipGetLastError());
    c->have_grid = true;
    return I3D_OK;
}
}  // namespace i3d

using namespace i3d;

extern "C" {

int i3d_set_grid(i3d_context* c, const i3d_grid_view* gv) {
    CTX_ENTER(c, gv && gv->num_voxels > 0 && gv->keys && gv->sdf && gv->sdf_refined && gv->albedo && gv->weight && gv->color,
              ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_grid: null grid or empty voxel list"));
    if (gv->num_voxels > (1ll << 30)) return ctx_fail(c, I3D_ERR_CAPACITY, "i3d_set_grid: more than 2^30 voxels");
    const size_t N = (size_t)gv->num_voxels;
    GridStaging g;     // the caller's record on the device (set_grid_device synchronises before it returns)
    CTX_HIP(c, g.alloc(N));
    CTX_HIP(c, ctx_upload(c, g.kxyz.p, gv->keys, 3 * N)); CTX_HIP(c, ctx_upload(c, g.sdf.p, gv->sdf, N)); CTX_HIP(c, ctx_upload(c, g.sdf_ref.p, gv->sdf_refined, N));
    CTX_HIP(c, ctx_upload(c, g.alb.p, gv->albedo, N)); CTX_HIP(c, ctx_upload(c, g.w.p, gv->weight, N)); CTX_HIP(c, ctx_upload(c, g.rgb.p, gv->color, 3 * N));
    return set_grid_device(c, (int)N, gv->voxel_size, gv->truncation, g);
}

int i3d_get_grid(i3d_context* c, double* sdf_refined, double* albedo) {
    CTX_ENTER(c, c->have_grid, ctx_fail(c, I3D_ERR_STATE, "i3d_get_grid: no grid"));
    const int N = c->N;
    DevBuf<double> a, b; CTX_HIP(c, a.alloc(N)); CTX_HIP(c, b.alloc(N));
    launch_gather_visit(c->stream, N, c->rank.p, c->x_sdf.p, c->x_alb.p, a.p, b.p);
    if (sdf_refined) CTX_HIP(c, ctx_download(c, sdf_refined, a.p, (size_t)N));
    if (albedo) CTX_HIP(c, ctx_download(c, albedo, b.p, (size_t)N));
    CTX_HIP(c, ctx_sync(c));
    return I3D_OK;
}

int i3d_update_grid(i3d_context* c, const double* sdf_refined, const double* albedo, const uint8_t* color) {
    CTX_ENTER(c, c->have_grid, ctx_fail(c, I3D_ERR_STATE, "i3d_update_grid: no grid"));
    const size_t N = (size_t)c->N;
    DevBuf<double> a, b; DevBuf<uint8_t> col;
    if (sdf_refined) { CTX_HIP(c, a.alloc(N)); CTX_HIP(c, ctx_upload(c, a.p, sdf_refined, N)); }
    if (albedo) { CTX_HIP(c, b.alloc(N)); CTX_HIP(c, ctx_upload(c, b.p, albedo, N)); }
    if (color) { CTX_HIP(c, col.alloc(3 * N)); CTX_HIP(c, ctx_upload(c, col.p, color, 3 * N)); }
    launch_update_fields(c->stream, c->N, c->rank.p, a.p, b.p, col.p, c->x_sdf.p, c->x_alb.p, c->f_sdf.p, c->f_alb.p, c->color.p);
    CTX_HIP(c, ctx_sync(c));
    c->assembled = false;
    return I3D_OK;
}

int i3d_set_voxel_sh(i3d_context* c, const double* voxel_sh) {
    CTX_ENTER(c, voxel_sh, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_voxel_sh: null pointer"));
    if (!c->have_grid) return ctx_fail(c, I3D_ERR_STATE, "i3d_set_voxel_sh: no grid");
    DevBuf<double> tmp; CTX_HIP(c, tmp.alloc((size_t)9 * c->N));
    CTX_HIP(c, ctx_upload(c, tmp.p, voxel_sh, (size_t)9 * c->N));
    launch_scatter_sh(c->stream, c->N, c->rank.p, tmp.p, c->sh.p);
    CTX_HIP(c, ctx_sync(c));
    c->have_sh = true;
    return I3D_OK;
}
int i3d_get_voxel_sh(i3d_context* c, double* out) {
    CTX_ENTER(c, out, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_get_voxel_sh: null pointer"));
    if (!c->have_grid) return ctx_fail(c, I3D_ERR_STATE, "i3d_get_voxel_sh: no grid");
    const int N = c->N;
    std::vector<float> sh((size_t)9 * N); VisitOrder vo;
    CTX_HIP(c, ctx_download(c, sh.data(), c->sh.p, sh.size()));
    if (int rc = vo.fetch(c, false)) return rc;
    CTX_HIP(c, ctx_sync(c));
    for (int s = 0; s < N; ++s) for (int j = 0; j < 9; ++j) out[(size_t)vo.rank[s] * 9 + j] = (double)sh[(size_t)j * N + s];
    return I3D_OK;
}

int i3d_grid_info(i3d_context* c, int64_t* num_voxels, float* voxel_size, float* truncation) {
    CTX_ENTER(c, c->have_grid, ctx_fail(c, I3D_ERR_STATE, "i3d_grid_info: no grid"));
    if (num_voxels) *num_voxels = c->N; if (voxel_size) *voxel_size = c->voxel_size; if (truncation) *truncation = c->truncation;
    return I3D_OK;
}
int i3d_export_grid(i3d_context* c, int32_t* keys, double* sdf, double* sdf_refined, double* albedo, float* weight, uint8_t* color) {
    CTX_ENTER(c, c->have_grid, ctx_fail(c, I3D_ERR_STATE, "i3d_export_grid: no grid"));
    const size_t N = (size_t)c->N;
    DevBuf<int> inv; GridStaging s;
    CTX_HIP(c, s.alloc(N));
    if (int rc = inverse_rank(c, inv)) return rc;
    launch_export_visit(c->stream, c->grid_view(), inv.p, nullptr, nullptr, s.view());
    if (keys) CTX_HIP(c, ctx_download(c, keys, s.kxyz.p, 3 * N));
    if (sdf) CTX_HIP(c, ctx_download(c, sdf, s.sdf.p, N));
    if (sdf_refined) CTX_HIP(c, ctx_download(c, sdf_refined, s.sdf_ref.p, N));
    if (albedo) CTX_HIP(c, ctx_download(c, albedo, s.alb.p, N));
    if (weight) CTX_HIP(c, ctx_download(c, weight, s.w.p, N));
    if (color) CTX_HIP(c, ctx_download(c, color, s.rgb.p, 3 * N));
    CTX_HIP(c, ctx_sync(c));
    return I3D_OK;
}

// SparseVoxelGrid<Voxel>::load (sparse_voxel_grid.cpp:545-568, records inserted in file order) followed by SDFAlgorithms::convert
// (algorithms.cpp:47-72: re-insertion in the Voxel map's iteration order, sdf_refined = sdf, albedo = 0.6, then clearInvalidVoxels)
int i3d_set_grid_from_tsdf_records(i3d_context* c, float voxel_size, int64_t n, const int32_t* keys, const float* sdf, const float* weight, const uint8_t* color) {
    CTX_ENTER(c, n > 0 && keys && sdf && weight && color, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_grid_from_tsdf_records: bad arguments"));
    // map 1: file order -> Voxel map (later records with the same key overwrite the payload, the node keeps its place)
    std::vector<int> o1;
    map_iteration_order_replay(keys, (size_t)n, o1, false);
    // map 2: VoxelSBR map filled in that order; invalid voxels (weight <= 0) are erased afterwards (order of the rest is unchanged)
    std::vector<int> k2(3 * o1.size()), o2(o1.size());
    for (size_t v = 0; v < o1.size(); ++v) for (int a = 0; a < 3; ++a) k2[3 * v + a] = keys[3 * (size_t)o1[v] + a];
    {   // distinct keys now: on the device (map_order.hip)
        DevBuf<int> dk, dord; CTX_HIP(c, dk.alloc(k2.size())); CTX_HIP(c, dord.alloc(o1.size()));
        CTX_HIP(c, ctx_upload(c, dk.p, k2.data(), k2.size()));
        const std::vector<MapEpoch> ep = map_epochs(o1.size());
        CTX_HIP(c, map_order_device(c->stream, dk.p, o1.size(), ep.data(), (int)ep.size(), dord.p));
        CTX_HIP(c, ctx_download(c, o2.data(), dord.p, o2.size()));
        CTX_HIP(c, ctx_sync(c));
    }
    std::vector<int32_t> k; std::vector<double> s, a; std::vector<float> w; std::vector<uint8_t> col;
    for (size_t v = 0; v < o2.size(); ++v) {
        const size_t i = (size_t)o1[(size_t)o2[v]];
        if (!(weight[i] > 0.0f)) continue;
        k.push_back(keys[3 * i]); k.push_back(keys[3 * i + 1]); k.push_back(keys[3 * i + 2]);
        s.push_back((double)sdf[i]); a.push_back(0.6); w.push_back(weight[i]);
        col.push_back(color[3 * i]); col.push_back(color[3 * i + 1]); col.push_back(color[3 * i + 2]);
    }
    if (w.empty()) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_grid_from_tsdf_records: no valid voxel");
    i3d_grid_view gv; gv.num_voxels = (int64_t)w.size(); gv.voxel_size = voxel_size; gv.truncation = voxel_size * 5.0f;
    gv.keys = k.data(); gv.sdf = s.data(); gv.sdf_refined = s.data(); gv.albedo = a.data(); gv.weight = w.data(); gv.color = col.data();
    return i3d_set_grid(c, &gv);
}

}  // extern "C"
