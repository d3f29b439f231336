// What the translation units of the fusion volume share (fusion.cpp: the table, the frames, merge, finish and the entry points on the model view;
// fusion_register_volume.cpp: DESIGN.md section 28; fusion_mesh.cpp: section 29; fusion_components.cpp: section 39): the handle, its error protocol, the volume as a model (model.hpp), and the slot list.
#pragma once
#include "../../../include/intrinsic3d_hip.h"
#include "../device/fusion_kernels.hpp"
#include "../device/slot_list.hpp"
#include "../device/fusion_mesh_kernels.hpp"
#include "../device/fusion_components_kernels.hpp"
#include "context.hpp"
#include "mesh_internal.hpp"
#include <functional>
#include <string>
#include <vector>

namespace i3d {

// The selected slots of a table as a sorted list, with the grown-only buffers of every user of one handle: flag and exclusive scan over
// the slots, the count, gather and radix sort of (64-bit key, 32-bit payload) over 64 bits.  All work is enqueued on the stream given to scan(); only count()
// synchronises it.  A list is valid until the next scan() on the same SlotList.
struct SlotList {
    // flag one lane per slot of t and scan the flags; remembers how to gather what sel selects
    template <class Sel> hipError_t scan(hipStream_t st, const FusionTable& t, const Sel& sel) {
        gather = [this, st, t, sel](size_t n) { launch_slot_gather(st, t, sel, flags.p, offs.p, (long long)n, key0.p, pay0.p); };
        stream = st; slots = (size_t)t.mask + 1;
        if (hipError_t e = flags.alloc(slots)) return e;
        if (hipError_t e = offs.alloc(slots)) return e;
        launch_slot_flag(st, t, sel, flags.p);
        return scan_flags();
    }
    hipError_t count(size_t& n);          // the length of the list: the last flag plus the last offset; one stream synchronisation
    hipError_t sort(size_t n);            // n > 0, the length (count(), or what the caller knows it to be): keys() / payload() in ascending key
    const unsigned long long* keys() const { return key1.p; }
    const unsigned int* payload() const { return pay1.p; }

private:
    hipError_t scan_flags();
    DevBuf<int> flags, offs; DevBuf<unsigned long long> key0, key1; DevBuf<unsigned int> pay0, pay1; DevBuf<char> temp;
    hipStream_t stream = nullptr; size_t slots = 0;
    std::function<void(size_t n)> gather;
};

}  // namespace i3d

struct i3d_fusion {
    int device = 0; hipStream_t stream = nullptr;
    float voxel_size = 0, truncation = 0, depth_min = 0, depth_max = 0, weight_sample = 10.0f;      // sparse_voxel_grid.cpp:44-51
    float clip[6] = {0, 0, 0, 0, 0, 0}; bool use_clip = false;
    unsigned long long capacity = 0, frames = 0;      // frames: integrate operations so far = the next ordinal (it feeds the rank and is never decremented)
    std::vector<bool> live;                           // per ordinal: the frame is in the volume (integrate marks, deintegrate / reintegrate clear)
    i3d::DevBuf<unsigned long long> keys, rank, crank; i3d::DevBuf<float> sdf, weight; i3d::DevBuf<uchar4> color;
    i3d::DevBuf<unsigned long long> d_count; i3d::DevBuf<int> d_flag;
    i3d::DevBuf<float> d_depth_raw, d_depth, d_normals; i3d::DevBuf<uint8_t> d_bgr;
    // result of finish(), or of snapshot(): have_snapshot = the records below are those of the last snapshot of the open volume
    bool finished = false, corrected = false;      // corrected: correctSDF has been written into the table (finish is not re-runnable past that point)
    bool have_snapshot = false;
    std::vector<int32_t> out_keys; std::vector<float> out_sdf, out_weight; std::vector<uint8_t> out_color;
    unsigned long long allocated = 0; int correct_launches = 0;
    // the volume as a model (model.hpp): what the drivers that read the stored field keep between calls.  Its brick bitmap is dropped by whatever changes the
    // table's weights or values (integrate, deintegrate, reintegrate, merge, a prune that removes something, finish, the debug poke); positional: a growth alone keeps it
    i3d::ModelBuffers model;
    // the sorted list of selected slots that finish, merge, register_volume (of the volume registered against, over src's table) and extract_mesh each build for
    // themselves: one set of buffers, grown only
    i3d::SlotList list;
    i3d::DevBuf<unsigned char> register_volume_scratch;      // volume-to-volume registration, in the handle of the volume registered against: slab | state
    i3d::DevBuf<unsigned long long> merge_counts;            // i3d_fusion_merge: its two counts
    i3d::DevBuf<unsigned long long> prune_counts;            // i3d_fusion_prune: its five counts
    // i3d_fusion_extract_mesh: the list's inverse map [capacity], the counters, the per-list-entry scratch and the device mesh, grown only; the
    // triangle table, uploaded once; the last mesh
    i3d::DevBuf<int> mesh_pos_of_slot; i3d::DevBuf<i3d::FusionMeshCounters> mesh_counters; i3d::DevBuf<unsigned char> mesh_list, mesh_out;
    i3d::DevBuf<unsigned char> mesh_ntri; i3d::DevBuf<signed char> mesh_tri; bool mesh_tables_ok = false;
    i3d::MeshData mesh; bool have_mesh = false;
    // i3d_fusion_components / i3d_fusion_prune_components: the counters, the per-node scratch, the components' sort keys and the sort's temp, the
    // byte per slot of a removal, grown only; nothing of it is read by a later call.  The list's inverse map is mesh_pos_of_slot, rebuilt by every call of either
    // user.  The last labelling, host copies as the last mesh
    i3d::DevBuf<i3d::FusionComponentCounters> comp_counters; i3d::DevBuf<unsigned char> comp_nodes, comp_sort, comp_remove;
    std::vector<int32_t> comp_keys, comp_label; std::vector<int64_t> comp_sizes; bool have_components = false;
    std::string error;
    i3d::FusionTable table() { return i3d::FusionTable{keys.p, sdf.p, weight.p, color.p, rank.p, crank.p, capacity - 1}; }
};

namespace i3d {

inline int fail(i3d_fusion* f, int code, const std::string& msg) { if (f) f->error = msg; return code; }
#define F_HIP(f, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(f, I3D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

// the table as the kernels that sample the field at points read it (queries, registration): no brick bitmap, nothing marches; and as the ray caster reads it
inline FusionRenderGrid field_grid(i3d_fusion* f) { return FusionRenderGrid{f->table(), (double)f->voxel_size, nullptr, {0, 0, 0}, {0, 0, 0}}; }
inline FusionRenderGrid fusion_grid(i3d_fusion* f) {
    const ModelBuffers::Bricks& k = f->model.bricks;
    return FusionRenderGrid{f->table(), (double)f->voxel_size, k.bits.p, {k.lo[0], k.lo[1], k.lo[2]}, {k.dim[0], k.dim[1], k.dim[2]}};
}

// the fusion volume as a model (model.hpp): fn names the entry point in the messages.  Its entry points refuse use_context_camera themselves, the fused colour is
// always there (no SH is involved), and its ray cast has no intensity plane
struct FusionModel final : Model {
    i3d_fusion* f;
    FusionModel(i3d_fusion* f_, const std::string& fn_)
        : Model(f_->model, f_->device, f_->stream, (double)f_->voxel_size, REGISTER_MAX_ROWS, "volume", "fusion", false, fn_), f(f_) {}
    int fail(int code, const std::string& msg) const override { return i3d::fail(f, code, msg); }
    int check_state(bool, const double*&, const double*&) const override { return I3D_OK; }
    int intensity_ready() const override { return I3D_OK; }
    size_t intensity_entries() const override { return (size_t)f->capacity; }      // the luminance of the fused colour per table slot
    void launch_intensity(double* vol) const override { launch_fusion_voxel_luminance(stream, f->table(), vol); }
    void brick_bounds(int* bounds) const override { launch_fusion_brick_bounds(stream, f->table(), bounds); }
    void brick_fill(unsigned* bits, const int lo[3], const int dim[3]) const override { launch_fusion_brick_fill(stream, f->table(), bits, lo, dim); }
    void cast(const RenderCam& cam, const RenderPlanes& out, RenderStatsDev* stats) const override { launch_render(stream, fusion_grid(f), cam, out, stats); }
    void cast_rays(const CastRays& p, RenderStatsDev* stats) const override { launch_cast_rays(stream, fusion_grid(f), p, stats); }
    void cast_color(const RenderCam& cam, const RenderColorPlanes& out, RenderStatsDev* stats) const override {
        launch_render_color(stream, fusion_grid(f), cam, out, stats);
    }
    void cast_rays_color(const CastRaysColor& p, RenderStatsDev* stats) const override { launch_cast_rays_color(stream, fusion_grid(f), p, stats); }
    void query(const QueryParams& p, const double* points, const QueryOut& out, QueryRow* rows, QueryRow* total) const override {
        launch_query(stream, field_grid(f), p, points, out, rows, total);
    }
    void register_pass(const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab) const override {
        launch_register(stream, field_grid(f), p, points, state, check_done, slab);
    }
    void track_sdf_pass(const TrackSdfParams& p, const TrackSdfPhoto* ph, const TrackSdfBatch& b, int check_done) const override {
        launch_track_sdf(stream, field_grid(f), p, ph, b, check_done);
    }
};

// the survivors of a removal moved into a fresh table (fusion.cpp): p's verdict and, where given, remove's byte per slot say who leaves
int prune_move(i3d_fusion* f, unsigned long long kept, bool shrink, const FusionPrune& p, const unsigned char* remove);
// the table still holds running means: frames and volumes can enter and leave
int table_open_check(i3d_fusion* f, const std::string& fn);
// what merge and register_volume ask of their two handles and of the motion between them (pose6 may be null: the identity); itself: "merged into" / "registered to"
int two_volumes_check(i3d_fusion* f, i3d_fusion* src, const std::string& fn, const double* pose6, const char* itself);

}  // namespace i3d
