// i3d_fusion_components / i3d_fusion_get_components / i3d_fusion_prune_components: the connected components of the stored voxels that pass criteria W and S, and
// the removal of the small ones (fusion_components_kernels.hip).  The nodes are a slot list (section 27.4, the node selector) with its
// inverse map; the union-find, the sizes and the numbering run on the list; the removal is the move of i3d_fusion_prune (prune_move, fusion.cpp) with one byte
// per slot as its verdict.
#include "fusion_internal.hpp"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace i3d;

namespace {

constexpr size_t COMPONENTS_MAX = 2147483647u;      // positions, labels and component numbers are int32

// what a labelling leaves: the host copies, and the device views that stay valid until the handle's list or node scratch is used again
struct Labelling {
    int64_t nodes = 0;
    std::vector<int32_t> keys, label; std::vector<int64_t> sizes;
    FusionNodeList list{nullptr, nullptr, nullptr, 0}; const int* d_label = nullptr;
};

int criteria_check(i3d_fusion* f, const std::string& fn, float min_weight, float max_abs_sdf, FusionPrune& p) {
    if (!std::isfinite(min_weight) || !std::isfinite(max_abs_sdf)) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": min_weight and max_abs_sdf must be finite");
    std::memset(&p, 0, sizeof(p));
    p.min_weight = min_weight; p.max_abs_sdf = max_abs_sdf; p.voxel_size = f->voxel_size;
    p.use_weight = min_weight >= 0.0f ? 1 : 0; p.use_sdf = max_abs_sdf > 0.0f ? 1 : 0; p.box_mode = 0;
    return I3D_OK;
}

// Section 39.2: the list and its inverse map, init, link, flatten, sizes, the sort of the components, the numbers.  Three synchronisations, whatever the volume:
// the list's length, the component count with the error word, the result.  with_nodes: keys and label are downloaded as well as the sizes.
int components_run(i3d_fusion* f, const std::string& fn, const FusionPrune& p, bool with_nodes, Labelling& L) {
    F_HIP(f, hipSetDevice(f->device));
    hipStream_t st = f->stream;
    const size_t cap = (size_t)f->capacity;
    const FusionTable t = f->table();
    auto pad = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    F_HIP(f, f->mesh_pos_of_slot.alloc(cap)); F_HIP(f, f->comp_counters.alloc(1));
    int* pos_of_slot = f->mesh_pos_of_slot.p; FusionComponentCounters* d_cnt = f->comp_counters.p;
    size_t n = 0;
    F_HIP(f, f->list.scan(st, t, SlotNode{p}));
    F_HIP(f, hipMemsetAsync(pos_of_slot, 0xFF, cap * sizeof(int), st));
    F_HIP(f, hipMemsetAsync(d_cnt, 0, sizeof(FusionComponentCounters), st));
    F_HIP(f, f->list.count(n));
    Labelling R;
    if (n == 0) { L = std::move(R); return I3D_OK; }
    if (n > COMPONENTS_MAX) return fail(f, I3D_ERR_CAPACITY, fn + ": " + std::to_string(n) + " nodes: more than 2^31 - 1");
    F_HIP(f, f->list.sort(n));
    launch_slot_positions(st, t, (long long)n, f->list.payload(), pos_of_slot);
    F_HIP(f, hipGetLastError());
    const FusionNodeList list{f->list.keys(), f->list.payload(), pos_of_slot, (int)n};
    // per node: parent | root | size | number of the root | label | key triple
    const size_t w = pad(n * 4), o_parent = 0, o_root = w, o_size = 2 * w, o_number = 3 * w, o_label = 4 * w, o_kxyz = 5 * w;
    F_HIP(f, f->comp_nodes.alloc(o_kxyz + pad(n * 12)));
    unsigned char* nb = f->comp_nodes.p;
    int* parent = (int*)(nb + o_parent); int* root = (int*)(nb + o_root); unsigned int* size = (unsigned int*)(nb + o_size);
    int* number = (int*)(nb + o_number); int* label = (int*)(nb + o_label); int* kxyz = (int*)(nb + o_kxyz);
    F_HIP(f, hipMemsetAsync(size, 0, n * 4, st));
    launch_fusion_components_init(st, list, parent);
    launch_fusion_components_link(st, t, list, parent, d_cnt);
    launch_fusion_components_flatten(st, (int)n, parent, root, d_cnt);
    launch_fusion_components_sizes(st, (int)n, root, size);
    F_HIP(f, hipGetLastError());
    FusionComponentCounters cnt;
    F_HIP(f, hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    if (cnt.error != 0 || cnt.roots == 0 || cnt.roots > n)
        return fail(f, I3D_ERR_HIP, fn + ": the union-find over " + std::to_string(n) + " nodes left its bounds (code " + std::to_string(cnt.error) + ", " +
                                        std::to_string(cnt.roots) + " roots): no labelling");
    const size_t C = (size_t)cnt.roots;
    size_t temp = 0;
    F_HIP(f, rocprim::radix_sort_keys(nullptr, temp, (unsigned long long*)nullptr, (unsigned long long*)nullptr, C, 0, 64, st));
    const size_t o_k0 = 0, o_k1 = pad(C * 8), o_sizes = 2 * pad(C * 8), o_temp = 3 * pad(C * 8);
    F_HIP(f, f->comp_sort.alloc(o_temp + pad(temp)));
    unsigned char* sb = f->comp_sort.p;
    unsigned long long* k0 = (unsigned long long*)(sb + o_k0); unsigned long long* k1 = (unsigned long long*)(sb + o_k1); long long* sizes = (long long*)(sb + o_sizes);
    launch_fusion_components_root_keys(st, (int)n, (long long)C, root, size, k0, d_cnt);
    F_HIP(f, hipGetLastError());
    F_HIP(f, rocprim::radix_sort_keys(sb + o_temp, temp, k0, k1, C, 0, 64, st));
    launch_fusion_components_number(st, (int)n, (long long)C, k1, number, sizes);
    launch_fusion_components_label(st, (int)n, root, number, label);
    F_HIP(f, hipGetLastError());
    R.nodes = (int64_t)n; R.sizes.resize(C);
    static_assert(sizeof(long long) == sizeof(int64_t), "the sizes are downloaded as they are");
    F_HIP(f, hipMemcpyAsync(R.sizes.data(), sizes, C * 8, hipMemcpyDeviceToHost, st));
    if (with_nodes) {
        launch_fusion_keys(st, t, (long long)n, list.slots, kxyz);
        F_HIP(f, hipGetLastError());
        R.keys.resize(n * 3); R.label.resize(n);
        F_HIP(f, hipMemcpyAsync(R.keys.data(), kxyz, n * 12, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipMemcpyAsync(R.label.data(), label, n * 4, hipMemcpyDeviceToHost, st));
    }
    F_HIP(f, hipStreamSynchronize(st));
    R.list = list; R.d_label = label;
    L = std::move(R);
    return I3D_OK;
}

}  // namespace

extern "C" {

int i3d_fusion_components(i3d_fusion* f, float min_weight, float max_abs_sdf, int64_t* counts3) {
    const std::string fn = "i3d_fusion_components";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    FusionPrune p;
    if (int rc = criteria_check(f, fn, min_weight, max_abs_sdf, p)) return rc;
    if (!counts3) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null counts3");
    Labelling L;
    if (int rc = components_run(f, fn, p, true, L)) return rc;
    counts3[0] = L.nodes; counts3[1] = (int64_t)L.sizes.size(); counts3[2] = L.sizes.empty() ? 0 : L.sizes[0];
    f->comp_keys = std::move(L.keys); f->comp_label = std::move(L.label); f->comp_sizes = std::move(L.sizes); f->have_components = true;
    return I3D_OK;
}

int i3d_fusion_get_components(i3d_fusion* f, int32_t* keys, int32_t* label, int64_t* sizes) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!f->have_components) return fail(f, I3D_ERR_STATE, "i3d_fusion_get_components: this volume has not been labelled (i3d_fusion_components)");
    if (keys && !f->comp_keys.empty()) std::memcpy(keys, f->comp_keys.data(), f->comp_keys.size() * sizeof(int32_t));
    if (label && !f->comp_label.empty()) std::memcpy(label, f->comp_label.data(), f->comp_label.size() * sizeof(int32_t));
    if (sizes && !f->comp_sizes.empty()) std::memcpy(sizes, f->comp_sizes.data(), f->comp_sizes.size() * sizeof(int64_t));
    return I3D_OK;
}

int i3d_fusion_prune_components(i3d_fusion* f, float min_weight, float max_abs_sdf, int64_t min_voxels, int64_t keep_largest, int32_t shrink, int64_t* counts5) {
    const std::string fn = "i3d_fusion_prune_components";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    FusionPrune p;
    if (int rc = criteria_check(f, fn, min_weight, max_abs_sdf, p)) return rc;
    if (min_voxels < 0 || keep_largest < 0) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": min_voxels and keep_largest must be >= 0 (0: off)");
    if (int rc = table_open_check(f, fn)) return rc;
    F_HIP(f, hipSetDevice(f->device));
    hipStream_t st = f->stream;
    unsigned long long stored = 0;
    F_HIP(f, hipMemcpyAsync(&stored, f->d_count.p, sizeof(stored), hipMemcpyDeviceToHost, st));      // arrives with the run's first synchronisation
    Labelling L;
    if (int rc = components_run(f, fn, p, false, L)) return rc;
    // the sizes descend with the number, so both rules remove a tail of the numbering: everything from `first` on
    const size_t C = L.sizes.size();
    size_t first = C;
    if (keep_largest > 0) first = std::min<size_t>(first, (size_t)std::min<int64_t>(keep_largest, (int64_t)C));
    if (min_voxels > 0) first = std::min<size_t>(first, (size_t)(std::partition_point(L.sizes.begin(), L.sizes.end(), [&](int64_t s) { return !(s < min_voxels); }) - L.sizes.begin()));
    unsigned long long removed = 0;
    for (size_t c = first; c < C; ++c) removed += (unsigned long long)L.sizes[c];
    if (removed > 0) {
        const size_t cap = (size_t)f->capacity;
        F_HIP(f, f->comp_remove.alloc(cap));
        F_HIP(f, hipMemsetAsync(f->comp_remove.p, 0, cap, st));
        launch_fusion_components_mark(st, L.list, f->capacity - 1, L.d_label, (int)first, f->comp_remove.p);
        F_HIP(f, hipGetLastError());
        FusionPrune none; std::memset(&none, 0, sizeof(none));          // every criterion off: the byte per slot is the verdict
        if (int rc = prune_move(f, stored - removed, shrink != 0, none, f->comp_remove.p)) return rc;
    }
    if (counts5) { counts5[0] = (int64_t)stored; counts5[1] = (int64_t)removed; counts5[2] = L.nodes; counts5[3] = (int64_t)C; counts5[4] = (int64_t)(C - first); }
    return I3D_OK;
}

}  // extern "C"
