// i3d_fusion_extract_mesh: an indexed, welded mesh of the fusion table as it stands (fusion_mesh_kernels.hip).  The stored voxels with a
// weight are a slot list (section 27.4, the weighted selector) with its inverse map; the two scans over the named vertices and the kept faces are the mesh's own.
#include "fusion_internal.hpp"
#include <rocprim/rocprim.hpp>
#include <algorithm>

using namespace i3d;

namespace {

constexpr long long FUSION_MESH_MAX = 2147483647ll;      // face indices and vertices are int32
static_assert(FUSION_MESH_TRI_STRIDE == MC_STRIDE, "the kernels read the triangle table with the row length host/mesh.cpp unpacks it to");

template <class T> struct MeshToLL { __host__ __device__ long long operator()(T v) const { return (long long)v; } };

int mesh_desc_check(i3d_fusion* f, const std::string& fn, const i3d_fusion_mesh_desc* d) {
    if (!d) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (!std::isfinite(d->min_weight) || d->min_weight < 0.0f) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": min_weight must be finite and >= 0");
    if (d->largest_component_only != 0 && d->largest_component_only != 1) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": largest_component_only must be 0 or 1");
    return I3D_OK;
}

// Section 29.2: the list and its slot -> position map, the count pass, the two scans, the vertices and the faces, one download.  Three
// synchronisations: the list's length, the two totals, the result.  M and out are written on success only.
int fusion_mesh_run(i3d_fusion* f, const std::string& fn, const i3d_fusion_mesh_desc* d, MeshData& M, i3d_fusion_mesh_stats& out) {
    F_HIP(f, hipSetDevice(f->device));
    hipStream_t st = f->stream;
    const size_t cap = (size_t)f->capacity;
    const FusionTable t = f->table();
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    if (!f->mesh_tables_ok) {
        const McTables& T = tables();
        F_HIP(f, f->mesh_ntri.alloc(256)); F_HIP(f, f->mesh_tri.alloc(256 * MC_STRIDE));
        F_HIP(f, hipMemcpyAsync(f->mesh_ntri.p, T.ntri, 256, hipMemcpyHostToDevice, st));
        F_HIP(f, hipMemcpyAsync(f->mesh_tri.p, T.tri, 256 * MC_STRIDE, hipMemcpyHostToDevice, st));
        F_HIP(f, hipStreamSynchronize(st));
        f->mesh_tables_ok = true;
    }
    F_HIP(f, f->mesh_pos_of_slot.alloc(cap)); F_HIP(f, f->mesh_counters.alloc(1));
    int* pos_of_slot = f->mesh_pos_of_slot.p; FusionMeshCounters* d_cnt = f->mesh_counters.p;
    size_t n = 0;
    F_HIP(f, f->list.scan(st, t, SlotWeighted{}));
    F_HIP(f, hipMemsetAsync(pos_of_slot, 0xFF, cap * sizeof(int), st));
    F_HIP(f, hipMemsetAsync(d_cnt, 0, sizeof(FusionMeshCounters), st));
    F_HIP(f, f->list.count(n));
    i3d_fusion_mesh_stats s; std::memset(&s, 0, sizeof(s));
    s.stored = (int64_t)n;
    MeshData R;
    if (n == 0) { M = std::move(R); out = s; return I3D_OK; }
    F_HIP(f, f->list.sort(n));
    const unsigned long long* k1 = f->list.keys(); const unsigned int* s1 = f->list.payload();
    launch_slot_positions(st, t, (long long)n, s1, pos_of_slot);
    F_HIP(f, hipGetLastError());
    // per list entry: kept | face offsets | used [6 n] | vertex ids [6 n] | scan temp
    const size_t nu = n * FUSION_MESH_CODES;
    using UsedIt = rocprim::transform_iterator<const unsigned char*, MeshToLL<unsigned char>, long long>;
    using KeptIt = rocprim::transform_iterator<const int*, MeshToLL<int>, long long>;
    size_t vscan_bytes = 0, fscan_bytes = 0;
    F_HIP(f, rocprim::exclusive_scan(nullptr, vscan_bytes, UsedIt(nullptr, MeshToLL<unsigned char>()), (long long*)nullptr, 0ll, nu, rocprim::plus<long long>(), st));
    F_HIP(f, rocprim::exclusive_scan(nullptr, fscan_bytes, KeptIt(nullptr, MeshToLL<int>()), (long long*)nullptr, 0ll, n, rocprim::plus<long long>(), st));
    const size_t temp = std::max(vscan_bytes, fscan_bytes);
    const size_t o_kept = 0, o_fat = o_kept + pad(n * 4), o_used = o_fat + pad(n * 8), o_vid = o_used + pad(nu), o_tmp1 = o_vid + pad(nu * 8);
    F_HIP(f, f->mesh_list.alloc(o_tmp1 + pad(temp)));
    unsigned char* lb = f->mesh_list.p;
    int* kept = (int*)(lb + o_kept); long long* face_at = (long long*)(lb + o_fat); unsigned char* used = lb + o_used; long long* vertex_id = (long long*)(lb + o_vid);
    F_HIP(f, hipMemsetAsync(used, 0, nu, st));
    const FusionMeshList list{k1, s1, pos_of_slot, (long long)n};
    launch_fusion_mesh_count(st, t, list, d->min_weight, f->voxel_size, f->mesh_ntri.p, f->mesh_tri.p, used, kept, d_cnt);
    F_HIP(f, hipGetLastError());
    { size_t bytes = temp; F_HIP(f, rocprim::exclusive_scan(lb + o_tmp1, bytes, UsedIt(used, MeshToLL<unsigned char>()), vertex_id, 0ll, nu, rocprim::plus<long long>(), st)); }
    { size_t bytes = temp; F_HIP(f, rocprim::exclusive_scan(lb + o_tmp1, bytes, KeptIt(kept, MeshToLL<int>()), face_at, 0ll, n, rocprim::plus<long long>(), st)); }
    long long vlast = 0, flast = 0; unsigned char ulast = 0; int klast = 0;
    F_HIP(f, hipMemcpyAsync(&vlast, vertex_id + (nu - 1), sizeof(long long), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(&ulast, used + (nu - 1), 1, hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(&flast, face_at + (n - 1), sizeof(long long), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(&klast, kept + (n - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    const long long nv = vlast + (long long)ulast, nf = flast + (long long)klast;
    if (nv > FUSION_MESH_MAX || 3 * nf > FUSION_MESH_MAX)
        return fail(f, I3D_ERR_CAPACITY, fn + ": " + std::to_string(nv) + " vertices and " + std::to_string(3 * nf) + " face indices: more than 2^31 - 1");
    FusionMeshCounters cnt;
    if (nv > 0) {
        const size_t o_v = 0, o_f = o_v + pad((size_t)nv * 12), o_c = o_f + pad((size_t)nf * 12);
        F_HIP(f, f->mesh_out.alloc(o_c + pad((size_t)nv * 3)));
        unsigned char* ob = f->mesh_out.p;
        launch_fusion_mesh_vertices(st, t, list, f->voxel_size, used, vertex_id, nv, (float*)(ob + o_v), ob + o_c, d_cnt);
        F_HIP(f, hipGetLastError());
        launch_fusion_mesh_faces(st, t, list, d->min_weight, f->voxel_size, f->mesh_ntri.p, f->mesh_tri.p, kept, vertex_id, face_at, nf, (int*)(ob + o_f));
        F_HIP(f, hipGetLastError());
        R.vertices.resize((size_t)nv * 3); R.colors.resize((size_t)nv * 3); R.faces.resize((size_t)nf * 3);
        F_HIP(f, hipMemcpyAsync(R.vertices.data(), ob + o_v, (size_t)nv * 12, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipMemcpyAsync(R.colors.data(), ob + o_c, (size_t)nv * 3, hipMemcpyDeviceToHost, st));
        if (nf > 0) F_HIP(f, hipMemcpyAsync(R.faces.data(), ob + o_f, (size_t)nf * 12, hipMemcpyDeviceToHost, st));
    }
    F_HIP(f, hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    s.valid_cells = (int64_t)cnt.valid_cells; s.surface_cells = (int64_t)cnt.surface_cells; s.raw_triangles = (int64_t)cnt.raw_triangles;
    s.corner_vertices = (int64_t)cnt.corner_vertices; s.degenerate_removed = (int64_t)cnt.degenerate_removed;
    s.rounded_corner_occurrences = (int64_t)cnt.rounded_corner_occurrences;
    if (d->largest_component_only) remove_loose_components(R);                      // host work, as on the context route (29.1 item 8)
    s.vertices = (int64_t)(R.vertices.size() / 3); s.faces = (int64_t)(R.faces.size() / 3);
    M = std::move(R); out = s;
    return I3D_OK;
}

}  // namespace

extern "C" {

void i3d_fusion_mesh_desc_default(i3d_fusion_mesh_desc* d) {
    if (!d) return;
    d->min_weight = 0.0f; d->largest_component_only = 0;
}

int i3d_fusion_extract_mesh(i3d_fusion* f, const i3d_fusion_mesh_desc* desc, int64_t* num_vertices, int64_t* num_faces, i3d_fusion_mesh_stats* stats) {
    const std::string fn = "i3d_fusion_extract_mesh";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (int rc = mesh_desc_check(f, fn, desc)) return rc;
    MeshData M; i3d_fusion_mesh_stats s;
    if (int rc = fusion_mesh_run(f, fn, desc, M, s)) return rc;
    f->mesh = std::move(M); f->have_mesh = true;
    if (num_vertices) *num_vertices = s.vertices;
    if (num_faces) *num_faces = s.faces;
    if (stats) *stats = s;
    return I3D_OK;
}

int i3d_fusion_get_mesh(i3d_fusion* f, float* vertices, uint8_t* colors, int32_t* faces) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!f->have_mesh) return fail(f, I3D_ERR_STATE, "i3d_fusion_get_mesh: no mesh has been extracted from this volume");
    const MeshData& M = f->mesh;
    if (vertices && !M.vertices.empty()) std::memcpy(vertices, M.vertices.data(), M.vertices.size() * sizeof(float));
    if (colors && !M.colors.empty()) std::memcpy(colors, M.colors.data(), M.colors.size());
    if (faces && !M.faces.empty()) std::memcpy(faces, M.faces.data(), M.faces.size() * sizeof(int32_t));
    return I3D_OK;
}

int i3d_fusion_export_mesh_ply(i3d_fusion* f, const i3d_fusion_mesh_desc* desc, const char* path) {
    const std::string fn = "i3d_fusion_export_mesh_ply";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (int rc = mesh_desc_check(f, fn, desc)) return rc;
    if (!path) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null path");
    MeshData M; i3d_fusion_mesh_stats s;
    if (int rc = fusion_mesh_run(f, fn, desc, M, s)) return rc;
    if (M.vertices.empty()) return fail(f, I3D_ERR_STATE, fn + ": the volume has no iso-surface, nothing to write");
    const int rc = i3d_write_ply(path, (int64_t)(M.vertices.size() / 3), M.vertices.data(), M.colors.data(), (int64_t)(M.faces.size() / 3), M.faces.data());
    if (rc) return fail(f, rc, fn + ": cannot write " + path);
    return I3D_OK;
}

}  // extern "C"
