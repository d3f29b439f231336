// TSDF fusion on the device — AppFusion::fuseSDF's volume (apps/src/app_fusion.cpp:107-200) behind a C handle.
//   i3d_fusion_integrate = erodeDiscontinuities + computeNormals + SparseVoxelGrid<Voxel>::integrate (alloc + update) for one frame
//   i3d_fusion_finish    = SDFAlgorithms::correctSDF + clearInvalidVoxels, and the reference's record order
//   i3d_fusion_merge     = a whole volume as one sample of the running mean under a rigid motion (none in the reference)
//   i3d_fusion_prune     = stored voxels dropped by weight, distance or box, the survivors moved into a fresh table (none in the reference; section 38)
//   i3d_fusion_insert_records / _load = SparseVoxelGrid::load / create(filename); i3d_fusion_snapshot = finish(0)'s records of the open volume (section 36)
// i3d_fusion_register_volume (the rigid motion that merge takes) is fusion_register_volume.cpp, i3d_fusion_extract_mesh (section 29)
// fusion_mesh.cpp; the handle and what the three files share is fusion_internal.hpp.
// The entry points that read the stored field (render, cast_rays, track, query_points, register_points, track_sdf) are the drivers of model.hpp on the volume's FusionModel.
// Frames are integrated in call order, one allocation launch and one integration launch per frame (fusion_kernels.hip).  The saved
// volume's record order is the iteration order of the reference's unordered_map; it is reproduced from the order of first insertion
// (a per-voxel rank kept by the allocation kernel; the stored slots sorted by it are a slot list, section 27.4) by replaying the insertions epoch by epoch on the device (map_order.hip) — the same replay levels.cpp uses for the level
// transitions.
#include "fusion_internal.hpp"
#include "../device/frame_math.hpp"
#include "map_order.hpp"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

using namespace i3d;

namespace {

// Matrix4f::inverse(): adjugate over determinant from the 2x2 minors of the row pairs, in float
void inverse4f(const float* m, float* inv) {
    const float s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3];
    const float s3 = m[1] * m[6] - m[5] * m[2], s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
    const float c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10];
    const float c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
    const float id = 1.0f / (((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0);
    inv[0] = ((m[5] * c5 - m[6] * c4) + m[7] * c3) * id;      inv[1] = ((-m[1] * c5 + m[2] * c4) - m[3] * c3) * id;
    inv[2] = ((m[13] * s5 - m[14] * s4) + m[15] * s3) * id;   inv[3] = ((-m[9] * s5 + m[10] * s4) - m[11] * s3) * id;
    inv[4] = ((-m[4] * c5 + m[6] * c2) - m[7] * c1) * id;     inv[5] = ((m[0] * c5 - m[2] * c2) + m[3] * c1) * id;
    inv[6] = ((-m[12] * s5 + m[14] * s2) - m[15] * s1) * id;  inv[7] = ((m[8] * s5 - m[10] * s2) + m[11] * s1) * id;
    inv[8] = ((m[4] * c4 - m[5] * c2) + m[7] * c0) * id;      inv[9] = ((-m[0] * c4 + m[1] * c2) - m[3] * c0) * id;
    inv[10] = ((m[12] * s4 - m[13] * s2) + m[15] * s0) * id;  inv[11] = ((-m[8] * s4 + m[9] * s2) - m[11] * s0) * id;
    inv[12] = ((-m[4] * c3 + m[5] * c1) - m[6] * c0) * id;    inv[13] = ((m[0] * c3 - m[1] * c1) + m[2] * c0) * id;
    inv[14] = ((-m[12] * s3 + m[13] * s1) - m[14] * s0) * id; inv[15] = ((m[8] * s3 - m[9] * s1) + m[10] * s0) * id;
}

}  // namespace

namespace i3d {

int table_open_check(i3d_fusion* f, const std::string& fn) {
    if (f->finished || f->corrected) return fail(f, I3D_ERR_STATE, fn + ": the volume has been finished (or a finish failed after correcting the table)");
    return I3D_OK;
}

int two_volumes_check(i3d_fusion* f, i3d_fusion* src, const std::string& fn, const double* pose6, const char* itself) {
    if (!src) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null source volume");
    if (f == src) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": a volume cannot be " + itself + " itself");
    if (f->device != src->device) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": the volumes are on different devices");
    return pose6 ? FusionModel(f, fn).check_pose(pose6) : I3D_OK;
}

// the two rocprim calls of a SlotList: the temp-size query, the grown-only temp, the call itself
hipError_t SlotList::scan_flags() {
    size_t bytes = 0;
    if (hipError_t e = rocprim::exclusive_scan(nullptr, bytes, flags.p, offs.p, 0, slots, rocprim::plus<int>(), stream)) return e;
    if (hipError_t e = temp.alloc(bytes)) return e;
    return rocprim::exclusive_scan(temp.p, bytes, flags.p, offs.p, 0, slots, rocprim::plus<int>(), stream);
}
hipError_t SlotList::count(size_t& n) {
    int last[2] = {0, 0};
    if (hipError_t e = hipMemcpyAsync(&last[0], flags.p + (slots - 1), sizeof(int), hipMemcpyDeviceToHost, stream)) return e;
    if (hipError_t e = hipMemcpyAsync(&last[1], offs.p + (slots - 1), sizeof(int), hipMemcpyDeviceToHost, stream)) return e;
    if (hipError_t e = hipStreamSynchronize(stream)) return e;
    n = (size_t)last[0] + (size_t)last[1];
    return hipSuccess;
}
hipError_t SlotList::sort(size_t n) {
    size_t bytes = 0;
    if (hipError_t e = key0.alloc(n)) return e;
    if (hipError_t e = key1.alloc(n)) return e;
    if (hipError_t e = pay0.alloc(n)) return e;
    if (hipError_t e = pay1.alloc(n)) return e;
    if (hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, key0.p, key1.p, pay0.p, pay1.p, n, 0, 64, stream)) return e;
    if (hipError_t e = temp.alloc(bytes)) return e;
    gather(n);
    if (hipError_t e = hipGetLastError()) return e;
    return rocprim::radix_sort_pairs(temp.p, bytes, key0.p, key1.p, pay0.p, pay1.p, n, 0, 64, stream);
}

}  // namespace i3d

namespace {

int alloc_table(i3d_fusion* f, unsigned long long cap, DevBuf<unsigned long long>& keys, DevBuf<unsigned long long>& rank, DevBuf<unsigned long long>& crank,
                DevBuf<float>& sdf, DevBuf<float>& weight, DevBuf<uchar4>& color) {
    F_HIP(f, keys.alloc(cap)); F_HIP(f, rank.alloc(cap)); F_HIP(f, crank.alloc(cap)); F_HIP(f, sdf.alloc(cap)); F_HIP(f, weight.alloc(cap)); F_HIP(f, color.alloc(cap));
    launch_fusion_clear(f->stream, FusionTable{keys.p, sdf.p, weight.p, color.p, rank.p, crank.p, cap - 1});
    return I3D_OK;
}
int grow(i3d_fusion* f) {
    if (f->capacity >= (1ull << 31)) return fail(f, I3D_ERR_CAPACITY, "fusion: more than 2^31 table slots");
    DevBuf<unsigned long long> keys, rank, crank; DevBuf<float> sdf, weight; DevBuf<uchar4> color;
    const unsigned long long cap = f->capacity * 2;
    const int rc = alloc_table(f, cap, keys, rank, crank, sdf, weight, color); if (rc) return rc;
    launch_fusion_rehash(f->stream, f->table(), FusionTable{keys.p, sdf.p, weight.p, color.p, rank.p, crank.p, cap - 1});
    F_HIP(f, hipStreamSynchronize(f->stream));
    f->keys = std::move(keys); f->rank = std::move(rank); f->crank = std::move(crank); f->sdf = std::move(sdf); f->weight = std::move(weight); f->color = std::move(color);
    f->capacity = cap;
    return I3D_OK;
}

// SparseVoxelGrid::computeFrustumBounds (sparse_voxel_grid.cpp:573-606); floor / ceil act on metres before the voxel conversion
void frustum_bounds(const i3d_fusion* f, const FusionCam& cam, const float* pose, int b[6]) {
    const int lo = std::numeric_limits<int>::min(), hi = std::numeric_limits<int>::max();
    b[0] = hi; b[1] = lo; b[2] = hi; b[3] = lo; b[4] = hi; b[5] = lo;
    const int px[4] = {0, cam.w - 1, cam.w - 1, 0}, py[4] = {0, 0, cam.h - 1, cam.h - 1};
    const float inv = 1.0f / f->voxel_size;
    auto to_voxel = [&](float v) { return (int)(v * inv + 0.5f); };
    for (int i = 0; i < 8; ++i) {
        const float depth = i < 4 ? f->depth_min : f->depth_max;
        float c[3] = {0, 0, 0};
        if (depth != 0.0f) { const float x = ((float)px[i & 3] - cam.cx) / cam.fx, y = ((float)py[i & 3] - cam.cy) / cam.fy; c[0] = depth * x; c[1] = depth * y; c[2] = depth; }
        for (int a = 0; a < 3; ++a) {
            const float pt = (pose[4 * a] * c[0] + (pose[4 * a + 1] * c[1] + pose[4 * a + 2] * c[2])) + pose[4 * a + 3];    // fixed-size Eigen product: halving reduction
            const int pl = to_voxel((float)(int)std::floor(pt)), pu = to_voxel((float)(int)std::ceil(pt));
            b[2 * a] = std::min(b[2 * a], std::min(pl, pu)); b[2 * a + 1] = std::max(b[2 * a + 1], std::max(pl, pu));
        }
    }
}

// ---- one frame's way into the kernels, shared by integrate / deintegrate / reintegrate and the sample lookup ----------------------------
struct FrameArgs { int32_t dw, dh; const float* dcam4; int32_t cw, ch; const float* ccam4; const float* depth; const uint8_t* bgr; int32_t erode_window; };
bool frame_args_ok(const FrameArgs& a) { return a.dw > 0 && a.dh > 0 && a.cw > 0 && a.ch > 0 && a.dcam4 && a.ccam4 && a.depth && a.bgr; }

// upload, erodeDiscontinuities and computeNormals into the handle's frame buffers
int upload_frame(i3d_fusion* f, const FrameArgs& a, FusionCam& dcam, FusionCam& ccam) {
    hipStream_t st = f->stream;
    const size_t dn = (size_t)a.dw * a.dh, cn = (size_t)a.cw * a.ch;
    F_HIP(f, f->d_depth_raw.alloc(dn)); F_HIP(f, f->d_depth.alloc(dn)); F_HIP(f, f->d_normals.alloc(dn * 3)); F_HIP(f, f->d_bgr.alloc(cn * 3));
    F_HIP(f, hipMemcpyAsync(f->d_depth_raw.p, a.depth, dn * sizeof(float), hipMemcpyHostToDevice, st));
    F_HIP(f, hipMemcpyAsync(f->d_bgr.p, a.bgr, cn * 3, hipMemcpyHostToDevice, st));
    dcam = FusionCam{a.dcam4[0], a.dcam4[1], a.dcam4[2], a.dcam4[3], a.dw, a.dh}; ccam = FusionCam{a.ccam4[0], a.ccam4[1], a.ccam4[2], a.ccam4[3], a.cw, a.ch};
    launch_erode(st, a.dw, a.dh, f->d_depth_raw.p, a.erode_window, 0.5f, f->d_depth.p);            // processing.h:57 default max_depth_diff
    launch_normals(st, dcam, f->d_depth.p, 0.3f, f->d_normals.p);                                  // processing.h:53 default depth_threshold
    return I3D_OK;
}

// the kernels' description of a frame at a pose: the volume's constants, both transforms, the frustum bounds, and the ordinal the rank carries
FusionFrame frame_of(const i3d_fusion* f, const FusionCam& dcam, const float* pose16, unsigned long long ordinal) {
    FusionFrame fr; std::memset(&fr, 0, sizeof(fr));
    fr.voxel_size = f->voxel_size; fr.truncation = f->truncation; fr.depth_min = f->depth_min; fr.depth_max = f->depth_max; fr.weight_sample = f->weight_sample;
    for (int i = 0; i < 6; ++i) fr.clip[i] = f->clip[i];
    fr.use_clip = f->use_clip ? 1 : 0; fr.frame = ordinal;
    std::memcpy(fr.c2w, pose16, sizeof(fr.c2w)); inverse4f(pose16, fr.w2c);
    frustum_bounds(f, dcam, pose16, fr.bounds);
    for (int i = 0; i < 6; ++i) if (fr.bounds[i] <= -FUSION_COORD_OFFSET + 2 || fr.bounds[i] >= FUSION_COORD_OFFSET - 2)
        fr.bounds[i] = fr.bounds[i] < 0 ? -FUSION_COORD_OFFSET + 2 : FUSION_COORD_OFFSET - 2;     // keys are packed in 21 bits per axis
    return fr;
}

// the limit / overflow protocol of an allocation: launch(limit) is idempotent, so it is repeated after a growth
template <class Launch>
int allocate_loop(i3d_fusion* f, Launch launch) {
    hipStream_t st = f->stream;
    for (;;) {
        F_HIP(f, hipMemsetAsync(f->d_flag.p, 0, sizeof(int), st));
        if (int rc = launch((unsigned long long)(0.6 * (double)f->capacity))) return rc;
        int overflow = 0;
        F_HIP(f, hipMemcpyAsync(&overflow, f->d_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        F_HIP(f, hipStreamSynchronize(st));
        if (overflow) { const int rc = grow(f); if (rc) return rc; continue; }
        // the in-kernel load test lags by the inserts of the waves in flight: keep the load factor of the finished frame below 0.6 as well
        unsigned long long have = 0;
        F_HIP(f, hipMemcpyAsync(&have, f->d_count.p, sizeof(have), hipMemcpyDeviceToHost, st));
        F_HIP(f, hipStreamSynchronize(st));
        if ((double)have <= 0.6 * (double)f->capacity) break;
        const int rc = grow(f); if (rc) return rc;         // rehash only: every cell of this frame already exists
        break;
    }
    return I3D_OK;
}
// SparseVoxelGrid::alloc of the uploaded frame
int allocate_frame(i3d_fusion* f, const FusionFrame& fr, const FusionCam& dcam) {
    return allocate_loop(f, [&](unsigned long long limit) {
        launch_fusion_alloc(f->stream, f->table(), fr, dcam, f->d_depth.p, limit, f->d_count.p, f->d_flag.p);
        return I3D_OK;
    });
}

// a frame can be taken out while the table still holds running means and the frame is in it
int live_check(i3d_fusion* f, const char* fn, uint64_t ordinal) {
    if (int rc = table_open_check(f, fn)) return rc;
    if (ordinal >= f->live.size() || !f->live[ordinal])
        return fail(f, I3D_ERR_STATE, std::string(fn) + ": ordinal " + std::to_string(ordinal) + " is not a frame of this volume (never integrated, or already taken out)");
    return I3D_OK;
}

// ---- the records of the volume in the reference's order: what finish, snapshot and the debug insertion order share -------------------
// the handle's slot list = the occupied slots sorted by first-insertion rank = the reference's insertion sequence; m = their number (written before any check)
int stored_by_rank(i3d_fusion* f, unsigned long long& m) {
    hipStream_t st = f->stream;
    F_HIP(f, f->list.scan(st, f->table(), SlotStored{}));
    F_HIP(f, hipMemcpyAsync(&m, f->d_count.p, sizeof(m), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    if (m > 0x7FFFFFFFull) return fail(f, I3D_ERR_CAPACITY, "fusion: more than 2^31 voxels");
    if (m > 0) F_HIP(f, f->list.sort((size_t)m));
    return I3D_OK;
}
struct Replay {
    unsigned long long m = 0;                       // stored voxels
    const unsigned int* slot_sorted = nullptr;      // the handle's slot list (valid until its next scan)
    DevBuf<unsigned int> visit_slot;                // [m] the slot of the v-th voxel of the map's iteration order
    DevBuf<int> pos_of_slot;                        // [capacity] v of a stored slot
};
// steps 1 and 2 of finish: the slot list by rank, then the insertions replayed (map_order.hip).  Empties the handle's records and sets `allocated`; m = 0 stops here
int replay_insertions(i3d_fusion* f, Replay& r) {
    hipStream_t st = f->stream; FusionTable t = f->table();
    const int rc = stored_by_rank(f, r.m);
    f->allocated = r.m;
    if (rc) return rc;
    const unsigned long long m = r.m;
    f->have_snapshot = false;
    f->out_keys.clear(); f->out_sdf.clear(); f->out_weight.clear(); f->out_color.clear();
    if (m == 0) return I3D_OK;
    r.slot_sorted = f->list.payload();
    DevBuf<int> kxyz; F_HIP(f, kxyz.alloc(3 * m));
    launch_fusion_keys(st, t, (long long)m, r.slot_sorted, kxyz.p);
    DevBuf<int> d_order;
    F_HIP(f, d_order.alloc(m)); F_HIP(f, r.pos_of_slot.alloc(f->capacity)); F_HIP(f, r.visit_slot.alloc(m));
    { const std::vector<MapEpoch> ep = map_epochs((size_t)m);                                            // keys of a hash table: distinct by construction
      F_HIP(f, map_order_device(st, kxyz.p, (size_t)m, ep.data(), (int)ep.size(), d_order.p)); }
    launch_fusion_positions(st, (long long)m, r.slot_sorted, d_order.p, r.visit_slot.p, r.pos_of_slot.p);
    return I3D_OK;
}
// step 4 of finish: clearInvalidVoxels' selection (weight > 0) and the records in iteration order, into the handle; r.m > 0
int export_records(i3d_fusion* f, const Replay& r, uint64_t& count) {
    hipStream_t st = f->stream; FusionTable t = f->table();
    const unsigned long long m = r.m;
    DevBuf<char> tmp; size_t bytes = 0;
    DevBuf<int> vflags, voffs;
    F_HIP(f, vflags.alloc(m)); F_HIP(f, voffs.alloc(m));
    launch_fusion_valid(st, t, (long long)m, r.visit_slot.p, vflags.p);
    F_HIP(f, rocprim::exclusive_scan(nullptr, bytes, vflags.p, voffs.p, 0, (size_t)m, rocprim::plus<int>(), st));
    F_HIP(f, tmp.alloc(bytes));
    F_HIP(f, rocprim::exclusive_scan(tmp.p, bytes, vflags.p, voffs.p, 0, (size_t)m, rocprim::plus<int>(), st));
    int last_off = 0, last_flag = 0;
    F_HIP(f, hipMemcpyAsync(&last_off, voffs.p + (m - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(&last_flag, vflags.p + (m - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    const size_t nv = (size_t)last_off + (size_t)last_flag;
    if (nv) {
        DevBuf<int> ok; DevBuf<float> os, ow; DevBuf<uint8_t> oc;
        F_HIP(f, ok.alloc(3 * nv)); F_HIP(f, os.alloc(nv)); F_HIP(f, ow.alloc(nv)); F_HIP(f, oc.alloc(3 * nv));
        launch_fusion_export(st, t, (long long)m, r.visit_slot.p, vflags.p, voffs.p, ok.p, os.p, ow.p, oc.p);
        f->out_keys.resize(3 * nv); f->out_sdf.resize(nv); f->out_weight.resize(nv); f->out_color.resize(3 * nv);
        F_HIP(f, hipMemcpyAsync(f->out_keys.data(), ok.p, sizeof(int) * 3 * nv, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipMemcpyAsync(f->out_sdf.data(), os.p, sizeof(float) * nv, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipMemcpyAsync(f->out_weight.data(), ow.p, sizeof(float) * nv, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipMemcpyAsync(f->out_color.data(), oc.p, 3 * nv, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipStreamSynchronize(st));
    }
    count = nv;
    return I3D_OK;
}

// on a refused load the volume is empty again: the table cleared, the count, the ordinal and its liveness reset
int unload(i3d_fusion* f) {
    launch_fusion_clear(f->stream, f->table());
    F_HIP(f, hipMemsetAsync(f->d_count.p, 0, sizeof(unsigned long long), f->stream));
    F_HIP(f, hipStreamSynchronize(f->stream));
    f->frames = 0; f->live.clear();
    return I3D_OK;
}

}  // namespace

namespace i3d {

// The move of a removal, for i3d_fusion_prune and i3d_fusion_prune_components: a fresh table for the `kept` survivors, no tombstones -
// an EMPTY home slot keeps meaning "not stored" (merge_sample) and the probe bound of insert_cell holds.  shrink: i3d_fusion_create's rule for initial_capacity =
// kept, never above the table there is (its load is below 0.6, the survivors are fewer).  Who leaves is p's verdict and, where given, the byte per slot.
int prune_move(i3d_fusion* f, unsigned long long kept, bool shrink, const FusionPrune& p, const unsigned char* remove) {
    hipStream_t st = f->stream;
    unsigned long long cap = f->capacity;
    if (shrink) { cap = 1ull << 12; while (cap < kept * 2 && cap < f->capacity) cap <<= 1; }
    DevBuf<unsigned long long> keys, rank, crank; DevBuf<float> sdf, weight; DevBuf<uchar4> color;
    if (int rc = alloc_table(f, cap, keys, rank, crank, sdf, weight, color)) return rc;       // the old table is intact
    if (kept > 0) launch_fusion_prune_rehash(st, f->table(), FusionTable{keys.p, sdf.p, weight.p, color.p, rank.p, crank.p, cap - 1}, p, remove);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(f->d_count.p, &kept, sizeof(kept), hipMemcpyHostToDevice, st));
    F_HIP(f, hipStreamSynchronize(st));               // the old table is read until here
    f->keys = std::move(keys); f->rank = std::move(rank); f->crank = std::move(crank); f->sdf = std::move(sdf); f->weight = std::move(weight); f->color = std::move(color);
    f->capacity = cap;
    f->model.bricks.ok = false;                      // voxels with a weight may have left
    return I3D_OK;
}

}  // namespace i3d

extern "C" {

int i3d_fusion_create(int32_t device_ordinal, float voxel_size, float depth_min, float depth_max, const float* clip6, uint64_t initial_capacity, i3d_fusion** out) {
    if (!out) return I3D_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (voxel_size <= 0.00001f) return I3D_ERR_INVALID_ARGUMENT;                   // SparseVoxelGrid::create returns nullptr
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_ordinal < 0 || device_ordinal >= ndev) return I3D_ERR_NO_DEVICE;
    if (hipSetDevice(device_ordinal) != hipSuccess) return I3D_ERR_NO_DEVICE;
    i3d_fusion* f = new i3d_fusion();
    f->device = device_ordinal; f->voxel_size = voxel_size; f->truncation = voxel_size * 5.0f; f->depth_min = depth_min; f->depth_max = depth_max;
    if (clip6) { float n = 0.0f; for (int i = 0; i < 6; ++i) { f->clip[i] = clip6[i]; n += clip6[i] * clip6[i]; } f->use_clip = std::sqrt(n) > 0.0f; }
    unsigned long long cap = 1ull << 12;
    while (cap < initial_capacity * 2 && cap < (1ull << 31)) cap <<= 1;
    f->capacity = cap;
    if (hipStreamCreate(&f->stream) != hipSuccess) { delete f; return I3D_ERR_HIP; }
    int rc = alloc_table(f, cap, f->keys, f->rank, f->crank, f->sdf, f->weight, f->color);
    if (rc == I3D_OK && (f->d_count.alloc(1) != hipSuccess || f->d_flag.alloc(2) != hipSuccess)) rc = I3D_ERR_HIP;
    if (rc == I3D_OK && hipMemsetAsync(f->d_count.p, 0, sizeof(unsigned long long), f->stream) != hipSuccess) rc = I3D_ERR_HIP;
    if (rc == I3D_OK && hipStreamSynchronize(f->stream) != hipSuccess) rc = I3D_ERR_HIP;
    if (rc != I3D_OK) { (void)hipStreamDestroy(f->stream); delete f; return rc; }
    *out = f;
    return I3D_OK;
}

void i3d_fusion_destroy(i3d_fusion* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    delete f;
}
const char* i3d_fusion_last_error(const i3d_fusion* f) { return f ? f->error.c_str() : "null fusion handle"; }

int i3d_fusion_integrate(i3d_fusion* f, int32_t dw, int32_t dh, const float* dcam4, int32_t cw, int32_t ch, const float* ccam4, const float* depth, const uint8_t* bgr,
                         const float* pose16, int32_t erode_window) {
    const char* fn = "i3d_fusion_integrate";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    const FrameArgs a{dw, dh, dcam4, cw, ch, ccam4, depth, bgr, erode_window};
    if (!frame_args_ok(a) || !pose16) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad arguments");
    if (int rc = table_open_check(f, fn)) return rc;
    F_HIP(f, hipSetDevice(f->device));
    f->model.bricks.ok = false;                     // the weights and values change
    hipStream_t st = f->stream;
    FusionCam dcam, ccam;
    if (int rc = upload_frame(f, a, dcam, ccam)) return rc;
    const FusionFrame fr = frame_of(f, dcam, pose16, f->frames);
    if (int rc = allocate_frame(f, fr, dcam)) return rc;
    launch_fusion_integrate(st, f->table(), fr, dcam, ccam, f->d_depth.p, f->d_normals.p, f->d_bgr.p);
    F_HIP(f, hipStreamSynchronize(st));                                                              // the host buffers may be reused by the caller
    f->live.push_back(true);
    ++f->frames;
    return I3D_OK;
}

int i3d_fusion_deintegrate(i3d_fusion* f, uint64_t ordinal, int32_t dw, int32_t dh, const float* dcam4, int32_t cw, int32_t ch, const float* ccam4, const float* depth,
                           const uint8_t* bgr, const float* pose16, int32_t erode_window) {
    const char* fn = "i3d_fusion_deintegrate";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    const FrameArgs a{dw, dh, dcam4, cw, ch, ccam4, depth, bgr, erode_window};
    if (!frame_args_ok(a) || !pose16) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad arguments");
    if (int rc = live_check(f, fn, ordinal)) return rc;
    F_HIP(f, hipSetDevice(f->device));
    f->model.bricks.ok = false;
    hipStream_t st = f->stream;
    FusionCam dcam, ccam;
    if (int rc = upload_frame(f, a, dcam, ccam)) return rc;
    launch_fusion_deintegrate(st, f->table(), frame_of(f, dcam, pose16, ordinal), dcam, ccam, f->d_depth.p, f->d_normals.p, f->d_bgr.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipStreamSynchronize(st));
    f->live[ordinal] = false;
    return I3D_OK;
}

int i3d_fusion_reintegrate(i3d_fusion* f, uint64_t ordinal, int32_t dw, int32_t dh, const float* dcam4, int32_t cw, int32_t ch, const float* ccam4, const float* depth,
                           const uint8_t* bgr, const float* old_pose16, int32_t erode_window, const float* new_pose16, uint64_t* new_ordinal) {
    const char* fn = "i3d_fusion_reintegrate";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    const FrameArgs a{dw, dh, dcam4, cw, ch, ccam4, depth, bgr, erode_window};
    if (!frame_args_ok(a) || !old_pose16 || !new_pose16) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad arguments");
    if (int rc = live_check(f, fn, ordinal)) return rc;
    F_HIP(f, hipSetDevice(f->device));
    f->model.bricks.ok = false;
    hipStream_t st = f->stream;
    FusionCam dcam, ccam;
    if (int rc = upload_frame(f, a, dcam, ccam)) return rc;
    const FusionFrame out = frame_of(f, dcam, old_pose16, ordinal), in = frame_of(f, dcam, new_pose16, f->frames);
    if (int rc = allocate_frame(f, in, dcam)) return rc;       // cells of the new pose carry the new ordinal: the subtracting half of the pass skips them
    launch_fusion_reintegrate(st, f->table(), out, in, dcam, ccam, f->d_depth.p, f->d_normals.p, f->d_bgr.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipStreamSynchronize(st));
    f->live[ordinal] = false; f->live.push_back(true);
    if (new_ordinal) *new_ordinal = f->frames;
    ++f->frames;
    return I3D_OK;
}

// f <- f (+) T(src): a whole volume as the sample of the running weighted mean
int i3d_fusion_merge(i3d_fusion* f, i3d_fusion* src, const double* pose6, i3d_merge_stats* stats) {
    const std::string fn = "i3d_fusion_merge";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (int rc = two_volumes_check(f, src, fn, pose6, "merged into")) return rc;
    if (std::memcmp(&f->voxel_size, &src->voxel_size, sizeof(float)) != 0 || std::memcmp(&f->truncation, &src->truncation, sizeof(float)) != 0)
        return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": the volumes must have the same voxel size and truncation, bit for bit");
    if (int rc = table_open_check(f, fn)) return rc;

    // the motion as the kernels use it.  Aligned: no rotation and a translation by whole voxels
    FusionMerge mg; std::memset(&mg, 0, sizeof(mg));
    mg.R[0] = mg.R[4] = mg.R[8] = 1.0;
    bool aligned = true;
    if (pose6) {
        aligned = pose6[0] == 0.0 && pose6[1] == 0.0 && pose6[2] == 0.0;
        for (int a = 0; a < 3; ++a) {
            mg.t[a] = pose6[3 + a]; mg.tv[a] = pose6[3 + a] / (double)f->voxel_size;
            aligned = aligned && std::trunc(mg.tv[a]) == mg.tv[a] && std::fabs(mg.tv[a]) < (double)FUSION_COORD_OFFSET;
        }
        if (!aligned) { FrameConst fc; fm::frame_from_pose(pose6, fc); for (int i = 0; i < 9; ++i) mg.R[i] = fc.hot.R[i]; }      // the register driver's R: x = R p + t
    }
    if (aligned) for (int a = 0; a < 3; ++a) mg.m[a] = (int)mg.tv[a];
    mg.voxel_size = f->voxel_size; mg.use_clip = f->use_clip ? 1 : 0; mg.ordinal = f->frames;
    for (int i = 0; i < 6; ++i) mg.clip[i] = f->clip[i];

    F_HIP(f, hipSetDevice(f->device));
    if (int rc = ensure_bricks(FusionModel(src, fn))) return fail(f, rc, fn + ": the source volume: " + src->error);
    F_HIP(f, hipStreamSynchronize(src->stream));                         // src is read on f's stream from here on
    i3d_merge_stats out; std::memset(&out, 0, sizeof(out));
    out.ordinal = f->frames; out.aligned = aligned ? 1 : 0;
    for (int i = 0; i < 9; ++i) out.rotation[i] = mg.R[i];
    for (int a = 0; a < 3; ++a) out.translation_voxels[a] = mg.tv[a];
    const ModelBuffers::Bricks& box = src->model.bricks;
    if (box.dim[0] > 0) {                                        // else nothing in src has a weight: no launch, the table is untouched
        hipStream_t st = f->stream;
        for (int a = 0; a < 3; ++a) { mg.lo[a] = box.lo[a] * (1 << RENDER_BRICK_SHIFT); mg.hi[a] = (box.lo[a] + box.dim[a]) * (1 << RENDER_BRICK_SHIFT); }
        f->model.bricks.ok = false;                                     // voxels appear, weights and values change
        unsigned long long before = 0, after = 0, counts[2] = {0, 0};
        F_HIP(f, f->merge_counts.alloc(2));
        F_HIP(f, hipMemcpyAsync(&before, f->d_count.p, sizeof(before), hipMemcpyDeviceToHost, st));
        if (int rc = allocate_loop(f, [&](unsigned long long limit) -> int {
                F_HIP(f, hipMemsetAsync(f->merge_counts.p, 0, 2 * sizeof(unsigned long long), st));
                launch_fusion_merge_alloc(st, f->table(), src->table(), mg, aligned, limit, f->d_count.p, f->d_flag.p, f->merge_counts.p);
                return I3D_OK;
            })) return rc;
        F_HIP(f, hipMemcpyAsync(&after, f->d_count.p, sizeof(after), hipMemcpyDeviceToHost, st));
        F_HIP(f, hipStreamSynchronize(st));
        const size_t n = (size_t)(after - before);
        if (n > 0) {                                                     // the final ranks: position among the inserted voxels in ascending order of packed key
            F_HIP(f, f->list.scan(st, f->table(), SlotInserted{mg.ordinal}));
            F_HIP(f, f->list.sort(n));
            launch_fusion_merge_rank(st, f->table(), mg.ordinal, (long long)n, f->list.payload());
        }
        launch_fusion_merge(st, f->table(), src->table(), mg, aligned, f->merge_counts.p);
        F_HIP(f, hipGetLastError());
        F_HIP(f, hipMemcpyAsync(counts, f->merge_counts.p, sizeof(counts), hipMemcpyDeviceToHost, st));
        F_HIP(f, hipStreamSynchronize(st));
        out.source_voxels = (int64_t)counts[0]; out.sampled = (int64_t)counts[1]; out.allocated = (int64_t)n;
    }
    f->live.push_back(false);                                            // the ordinal is consumed and never live: a merge cannot be taken out again
    ++f->frames;
    if (stats) *stats = out;
    return I3D_OK;
}

// stored voxels dropped by weight, distance or box; the survivors move into a fresh table
int i3d_fusion_prune(i3d_fusion* f, float min_weight, float max_abs_sdf, int32_t box_mode, const float* box6, int32_t shrink, int64_t* counts5) {
    const std::string fn = "i3d_fusion_prune";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(min_weight) || !std::isfinite(max_abs_sdf)) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": min_weight and max_abs_sdf must be finite");
    if (box_mode < 0 || box_mode > 2) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": box_mode must be 0 (no box), 1 (keep the inside) or 2 (erase the inside)");
    FusionPrune p; std::memset(&p, 0, sizeof(p));
    if (box_mode != 0) {
        if (!box6) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": box_mode != 0 needs a box (null box6)");
        for (int i = 0; i < 6; ++i) if (!std::isfinite(box6[i])) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": the box is not finite");
        for (int a = 0; a < 3; ++a) if (box6[2 * a] > box6[2 * a + 1]) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": the box has lo > hi on axis " + std::to_string(a));
        for (int i = 0; i < 6; ++i) p.box[i] = box6[i];
    }
    if (int rc = table_open_check(f, fn)) return rc;
    p.min_weight = min_weight; p.max_abs_sdf = max_abs_sdf; p.voxel_size = f->voxel_size;
    p.use_weight = min_weight >= 0.0f ? 1 : 0; p.use_sdf = max_abs_sdf > 0.0f ? 1 : 0; p.box_mode = box_mode;

    F_HIP(f, hipSetDevice(f->device));
    hipStream_t st = f->stream;
    unsigned long long counts[5] = {0, 0, 0, 0, 0};
    F_HIP(f, f->prune_counts.alloc(5));
    F_HIP(f, hipMemsetAsync(f->prune_counts.p, 0, sizeof(counts), st));
    launch_fusion_prune_count(st, f->table(), p, f->prune_counts.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(counts, f->prune_counts.p, sizeof(counts), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    if (counts[1] > 0)
        if (int rc = prune_move(f, counts[0] - counts[1], shrink != 0, p, nullptr)) return rc;
    if (counts5) for (int i = 0; i < 5; ++i) counts5[i] = (int64_t)counts[i];
    return I3D_OK;
}

int i3d_fusion_debug_voxels(i3d_fusion* f, int64_t n, const int32_t* keys, uint8_t* found, float* sdf, float* weight, uint8_t* color, int64_t* first_frame) {
    const char* fn = "i3d_fusion_debug_voxels";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (n < 0 || n > (1ll << 28) || (n > 0 && (!keys || !found || !sdf || !weight || !color || !first_frame))) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad arguments");
    if (n == 0) return I3D_OK;
    F_HIP(f, hipSetDevice(f->device));
    hipStream_t st = f->stream;
    const size_t m = (size_t)n;
    DevBuf<int> d_keys; DevBuf<uint8_t> d_found, d_rgb; DevBuf<float> d_sdf, d_w; DevBuf<long long> d_first;
    F_HIP(f, d_keys.alloc(3 * m)); F_HIP(f, d_found.alloc(m)); F_HIP(f, d_rgb.alloc(3 * m)); F_HIP(f, d_sdf.alloc(m)); F_HIP(f, d_w.alloc(m)); F_HIP(f, d_first.alloc(m));
    F_HIP(f, hipMemcpyAsync(d_keys.p, keys, 3 * m * sizeof(int32_t), hipMemcpyHostToDevice, st));
    launch_fusion_debug_voxels(st, f->table(), (long long)n, d_keys.p, d_found.p, d_sdf.p, d_w.p, d_rgb.p, d_first.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(found, d_found.p, m, hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(sdf, d_sdf.p, m * sizeof(float), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(weight, d_w.p, m * sizeof(float), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(color, d_rgb.p, 3 * m, hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(first_frame, d_first.p, m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    return I3D_OK;
}

int i3d_fusion_debug_frame_samples(i3d_fusion* f, int32_t dw, int32_t dh, const float* dcam4, int32_t cw, int32_t ch, const float* ccam4, const float* depth,
                                   const uint8_t* bgr, const float* pose16, int32_t erode_window, int64_t n, const int32_t* keys, uint8_t* on, float* sample, float* wu,
                                   uint8_t* has_color, uint8_t* rgb) {
    const char* fn = "i3d_fusion_debug_frame_samples";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    const FrameArgs a{dw, dh, dcam4, cw, ch, ccam4, depth, bgr, erode_window};
    if (!frame_args_ok(a) || !pose16 || n < 0 || n > (1ll << 28) || (n > 0 && (!keys || !on || !sample || !wu || !has_color || !rgb)))
        return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad arguments");
    if (n == 0) return I3D_OK;
    F_HIP(f, hipSetDevice(f->device));
    hipStream_t st = f->stream;
    FusionCam dcam, ccam;
    if (int rc = upload_frame(f, a, dcam, ccam)) return rc;
    const size_t m = (size_t)n;
    DevBuf<int> d_keys; DevBuf<uint8_t> d_on, d_has, d_rgb; DevBuf<float> d_sample, d_wu;
    F_HIP(f, d_keys.alloc(3 * m)); F_HIP(f, d_on.alloc(m)); F_HIP(f, d_has.alloc(m)); F_HIP(f, d_rgb.alloc(3 * m)); F_HIP(f, d_sample.alloc(m)); F_HIP(f, d_wu.alloc(m));
    F_HIP(f, hipMemcpyAsync(d_keys.p, keys, 3 * m * sizeof(int32_t), hipMemcpyHostToDevice, st));
    launch_fusion_debug_frame_samples(st, frame_of(f, dcam, pose16, 0), dcam, ccam, f->d_depth.p, f->d_normals.p, f->d_bgr.p, (long long)n, d_keys.p, d_on.p, d_sample.p,
                                      d_wu.p, d_has.p, d_rgb.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(on, d_on.p, m, hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(sample, d_sample.p, m * sizeof(float), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(wu, d_wu.p, m * sizeof(float), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(has_color, d_has.p, m, hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(rgb, d_rgb.p, 3 * m, hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    return I3D_OK;
}

int i3d_fusion_finish(i3d_fusion* f, int32_t correct_iterations, uint64_t* count) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (f->finished) { if (count) *count = f->out_sdf.size(); return I3D_OK; }
    if (f->corrected) return fail(f, I3D_ERR_STATE, "i3d_fusion_finish: an earlier finish failed after correctSDF had been written into the table; the volume cannot be finished twice");
    F_HIP(f, hipSetDevice(f->device));
    f->model.bricks.ok = false;                     // correctSDF writes values and weights
    hipStream_t st = f->stream; FusionTable t = f->table();
    const unsigned long long cap = f->capacity;
    // 1. + 2. the stored slots by first-insertion rank and the replay: iteration order of the reference's map
    Replay r;
    if (int rc = replay_insertions(f, r)) return rc;
    const unsigned long long m = r.m;
    if (m == 0) { f->finished = true; if (count) *count = 0; return I3D_OK; }
    DevBuf<char> tmp; size_t bytes = 0;                  // of the sort below, which is over a list, not over slots
    // 3. correctSDF: up to `correct_iterations` in-place sweeps, each evaluated as a fixed point (see k_correct), in a spatially sorted
    //    compact index space with the 26 neighbour indices resolved once
    if (correct_iterations > 0) {
        DevBuf<unsigned long long> sk0, sk1; DevBuf<unsigned int> slot_c; DevBuf<int> compact_of_slot, c_pos, nbr; DevBuf<float> c_sdf, c_cur;
        DevBuf<unsigned char> c_valid, c_touched, c_upd;
        F_HIP(f, sk0.alloc(m)); F_HIP(f, sk1.alloc(m)); F_HIP(f, slot_c.alloc(m)); F_HIP(f, compact_of_slot.alloc(cap)); F_HIP(f, c_pos.alloc(m));
        F_HIP(f, nbr.alloc(26 * m)); F_HIP(f, c_sdf.alloc(m)); F_HIP(f, c_cur.alloc(m)); F_HIP(f, c_valid.alloc(m)); F_HIP(f, c_touched.alloc(m)); F_HIP(f, c_upd.alloc(m));
        launch_fusion_spatial_keys(st, t, (long long)m, r.slot_sorted, sk0.p);
        bytes = 0;
        F_HIP(f, rocprim::radix_sort_pairs(nullptr, bytes, sk0.p, sk1.p, r.slot_sorted, slot_c.p, (size_t)m, 0, 64, st));
        F_HIP(f, tmp.alloc(bytes));
        F_HIP(f, rocprim::radix_sort_pairs(tmp.p, bytes, sk0.p, sk1.p, r.slot_sorted, slot_c.p, (size_t)m, 0, 64, st));
        launch_fusion_compact_init(st, t, (long long)m, slot_c.p, r.pos_of_slot.p, compact_of_slot.p, c_sdf.p, c_pos.p, c_valid.p, c_touched.p);
        launch_fusion_build_nbr(st, t, (long long)m, slot_c.p, compact_of_slot.p, c_valid.p, nbr.p);
        f->correct_launches = 0;
        for (int iter = 0; iter < correct_iterations; ++iter) {
            F_HIP(f, hipMemcpyAsync(c_cur.p, c_sdf.p, sizeof(float) * m, hipMemcpyDeviceToDevice, st));
            F_HIP(f, hipMemsetAsync(c_upd.p, 0, m, st));
            for (;;) {
                F_HIP(f, hipMemsetAsync(f->d_flag.p, 0, 2 * sizeof(int), st));
                launch_fusion_correct(st, t, (long long)m, f->voxel_size, slot_c.p, nbr.p, c_pos.p, c_valid.p, c_sdf.p, c_cur.p, c_upd.p, f->d_flag.p);
                int changed = 0;
                F_HIP(f, hipMemcpyAsync(&changed, f->d_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
                F_HIP(f, hipStreamSynchronize(st));
                ++f->correct_launches;
                if (!changed) break;
            }
            launch_fusion_commit(st, (long long)m, c_valid.p, c_cur.p, c_upd.p, c_sdf.p, c_touched.p, f->d_flag.p + 1);
            int has_update = 0;
            F_HIP(f, hipMemcpyAsync(&has_update, f->d_flag.p + 1, sizeof(int), hipMemcpyDeviceToHost, st));
            F_HIP(f, hipStreamSynchronize(st));
            if (!has_update) break;
        }
        f->corrected = true;                              // from here on the table holds corrected values: a retry would correct them twice
        launch_fusion_write_back(st, t, (long long)m, slot_c.p, c_sdf.p, c_touched.p);
        F_HIP(f, hipStreamSynchronize(st));
    }
    // 4. clearInvalidVoxels + records in iteration order
    uint64_t nv = 0;
    if (int rc = export_records(f, r, nv)) return rc;
    f->finished = true;                                  // only now: a failed finish can be diagnosed (i3d_fusion_last_error) and is not mistaken for an empty volume
    if (count) *count = nv;
    return I3D_OK;
}

int i3d_fusion_info(const i3d_fusion* f, uint64_t* frames, uint64_t* allocated, uint64_t* capacity, int32_t* correct_launches) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (frames) *frames = f->frames;
    if (allocated) *allocated = f->allocated;
    if (capacity) *capacity = f->capacity;
    if (correct_launches) *correct_launches = f->correct_launches;
    return I3D_OK;
}

int i3d_fusion_get(const i3d_fusion* f, int32_t* keys, float* sdf, float* weight, uint8_t* color) {
    if (!f || !(f->finished || f->have_snapshot)) return I3D_ERR_STATE;
    const size_t n = f->out_sdf.size();
    if (keys) std::memcpy(keys, f->out_keys.data(), sizeof(int32_t) * 3 * n);
    if (sdf) std::memcpy(sdf, f->out_sdf.data(), sizeof(float) * n);
    if (weight) std::memcpy(weight, f->out_weight.data(), sizeof(float) * n);
    if (color) std::memcpy(color, f->out_color.data(), 3 * n);
    return I3D_OK;
}

// ---- records into an empty volume, a volume from a file, the records of an open volume -------------------------------------------------
// SparseVoxelGrid::load's loop (sparse_voxel_grid.cpp:532-569): record i enters with the rank (0 << 41) | i, and the load is ordinal 0
int i3d_fusion_insert_records(i3d_fusion* f, uint64_t n, const int32_t* keys, const float* sdf, const float* weight, const uint8_t* color) {
    const std::string fn = "i3d_fusion_insert_records";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (n > (1ull << 30)) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": more than 2^30 records");
    if (n > 0 && (!keys || !sdf || !weight || !color)) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null argument");
    for (uint64_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) if (keys[3 * i + a] <= -FUSION_COORD_OFFSET || keys[3 * i + a] >= FUSION_COORD_OFFSET)
            return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": record " + std::to_string(i) + " has a key coordinate of magnitude >= 2^20");
        if (!std::isfinite(sdf[i])) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": record " + std::to_string(i) + " has a non-finite sdf");
        if (!std::isfinite(weight[i]) || weight[i] < 0.0f) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": record " + std::to_string(i) + " has a non-finite or negative weight");
    }
    if (int rc = table_open_check(f, fn)) return rc;
    F_HIP(f, hipSetDevice(f->device));
    hipStream_t st = f->stream;
    unsigned long long have = 0;
    F_HIP(f, hipMemcpyAsync(&have, f->d_count.p, sizeof(have), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    if (f->frames != 0 || have != 0) return fail(f, I3D_ERR_STATE, fn + ": the volume is not empty (records enter a volume that no load, integrate or merge has touched)");
    while (0.6 * (double)f->capacity < (double)n) if (int rc = grow(f)) return rc;            // the launch below never overflows
    f->model.bricks.ok = false;
    if (n > 0) {
        const size_t m = (size_t)n;
        DevBuf<int> d_keys; DevBuf<uint8_t> d_rgb; DevBuf<float> d_sdf, d_w;
        F_HIP(f, d_keys.alloc(3 * m)); F_HIP(f, d_rgb.alloc(3 * m)); F_HIP(f, d_sdf.alloc(m)); F_HIP(f, d_w.alloc(m));
        F_HIP(f, hipMemcpyAsync(d_keys.p, keys, 3 * m * sizeof(int32_t), hipMemcpyHostToDevice, st));
        F_HIP(f, hipMemcpyAsync(d_sdf.p, sdf, m * sizeof(float), hipMemcpyHostToDevice, st));
        F_HIP(f, hipMemcpyAsync(d_w.p, weight, m * sizeof(float), hipMemcpyHostToDevice, st));
        F_HIP(f, hipMemcpyAsync(d_rgb.p, color, 3 * m, hipMemcpyHostToDevice, st));
        F_HIP(f, hipMemsetAsync(f->d_flag.p, 0, 2 * sizeof(int), st));
        launch_fusion_insert_records(st, f->table(), (long long)n, d_keys.p, d_sdf.p, d_w.p, d_rgb.p, f->d_count.p, f->d_flag.p);
        F_HIP(f, hipGetLastError());
        int flags[2] = {0, 0};
        F_HIP(f, hipMemcpyAsync(flags, f->d_flag.p, sizeof(flags), hipMemcpyDeviceToHost, st));
        F_HIP(f, hipMemcpyAsync(&have, f->d_count.p, sizeof(have), hipMemcpyDeviceToHost, st));
        F_HIP(f, hipStreamSynchronize(st));                                                         // the host buffers may be reused by the caller
        if (have != n || flags[0] || flags[1]) {
            if (int rc = unload(f)) return rc;
            if (flags[1]) return fail(f, I3D_ERR_CAPACITY, fn + ": the table filled up");
            return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": a key appears twice (" + std::to_string(n - have) + " of " + std::to_string(n) + " records not stored); the volume is empty again");
        }
    }
    f->live.push_back(false);                                            // the load is ordinal 0 and never live: what it brought cannot be taken out
    ++f->frames;
    return I3D_OK;
}

// SparseVoxelGrid::create(filename, depth_min, depth_max) (sparse_voxel_grid.cpp:68-80): voxel size, truncation and integration weight sample are the file's.
// A weight sample of 0 - what i3d_tsdf_write's callers give when they have none - makes integrate use unit weights, as it does in the reference.
int i3d_fusion_load(int32_t device_ordinal, const char* path, float depth_min, float depth_max, const float* clip6, i3d_fusion** out) {
    if (!out) return I3D_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!path) return I3D_ERR_INVALID_ARGUMENT;
    float vs = 0, tr = 0, iw = 0, ml = 0; uint64_t n = 0;
    if (int rc = i3d_tsdf_read_header(path, &vs, &tr, &iw, &n, &ml)) return rc;
    if (!(vs > 0.00001f) || !std::isfinite(vs) || !std::isfinite(tr) || !(tr > 0.0f) || !std::isfinite(iw)) return I3D_ERR_IO;
    { std::ifstream file(path, std::ios::binary | std::ios::ate);             // a count the file cannot hold: refused before anything of that size is allocated
      if (!file.is_open()) return I3D_ERR_IO;
      const std::streamoff size = file.tellg();
      if (size < 24 || n > ((uint64_t)size - 24) / 24) return I3D_ERR_IO; }
    if (n > (1ull << 30)) return I3D_ERR_INVALID_ARGUMENT;
    std::vector<int32_t> keys(3 * (size_t)n + 3); std::vector<float> sdf((size_t)n + 1), weight((size_t)n + 1); std::vector<uint8_t> color(3 * (size_t)n + 3);
    if (int rc = i3d_tsdf_read_records(path, n, keys.data(), sdf.data(), weight.data(), color.data())) return rc;
    i3d_fusion* f = nullptr;
    if (int rc = i3d_fusion_create(device_ordinal, vs, depth_min, depth_max, clip6, n, &f)) return rc;
    f->truncation = tr; f->weight_sample = iw;
    if (int rc = i3d_fusion_insert_records(f, n, keys.data(), sdf.data(), weight.data(), color.data())) { i3d_fusion_destroy(f); return rc; }
    *out = f;
    return I3D_OK;
}

// the records i3d_fusion_finish(f, 0, ..) would produce, with the volume left open and its table untouched
int i3d_fusion_snapshot(i3d_fusion* f, uint64_t* count) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (f->finished) { if (count) *count = f->out_sdf.size(); return I3D_OK; }
    F_HIP(f, hipSetDevice(f->device));
    Replay r;
    if (int rc = replay_insertions(f, r)) return rc;
    uint64_t nv = 0;
    if (r.m > 0) if (int rc = export_records(f, r, nv)) return rc;
    f->have_snapshot = true;
    if (count) *count = nv;
    return I3D_OK;
}

// tests only: the stored keys in ascending rank = the insertion sequence the replay starts from
int i3d_fusion_debug_insertion_order(i3d_fusion* f, uint64_t capacity, int32_t* keys, uint64_t* count) {
    const char* fn = "i3d_fusion_debug_insertion_order";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!count || (capacity > 0 && !keys)) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null argument");
    F_HIP(f, hipSetDevice(f->device));
    unsigned long long m = 0;
    const int rc = stored_by_rank(f, m);
    *count = m;
    if (rc) return rc;
    if (capacity < m) return fail(f, I3D_ERR_CAPACITY, std::string(fn) + ": " + std::to_string(m) + " stored voxels, room for " + std::to_string(capacity));
    if (m == 0) return I3D_OK;
    DevBuf<int> kxyz; F_HIP(f, kxyz.alloc(3 * m));
    launch_fusion_keys(f->stream, f->table(), (long long)m, f->list.payload(), kxyz.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(keys, kxyz.p, 3 * m * sizeof(int32_t), hipMemcpyDeviceToHost, f->stream));
    F_HIP(f, hipStreamSynchronize(f->stream));
    return I3D_OK;
}

// what both views of the volume ask of their descriptor: a free camera of a size in range
static int fusion_view_check(i3d_fusion* f, const i3d_render_desc* d, const std::string& fn) {
    if (!d) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (d->frame != -1) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": desc->frame must be -1 (a free camera; the volume has no keyframes)");
    if (d->width <= 0 || d->height <= 0 || d->width > (1 << 15) || d->height > (1 << 15))             // as i3d_render_view
        return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": image size (desc->width / height) out of range");
    return I3D_OK;
}

int i3d_fusion_render(i3d_fusion* f, const i3d_render_desc* d, float* depth, float* normal, i3d_render_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (int rc = fusion_view_check(f, d, "i3d_fusion_render")) return rc;
    return render_run(FusionModel(f, "i3d_fusion_render"), render_cam(camera_of(d->intrinsics4, d->distortion5, d->width, d->height), d->pose6, d->min_depth, d->max_depth),
                      RenderWant{depth, normal, nullptr, nullptr, nullptr, nullptr}, nullptr, stats);
}

// the colour view of the volume: depth and the fused colour at the hit
int i3d_fusion_render_color(i3d_fusion* f, const i3d_render_desc* d, float* color, float* depth, i3d_render_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (int rc = fusion_view_check(f, d, "i3d_fusion_render_color")) return rc;
    return render_run(FusionModel(f, "i3d_fusion_render_color"), render_cam(camera_of(d->intrinsics4, d->distortion5, d->width, d->height), d->pose6, d->min_depth, d->max_depth),
                      RenderWant{depth, nullptr, nullptr, nullptr, nullptr, nullptr, color, true}, nullptr, stats);
}

int i3d_fusion_track(i3d_fusion* f, const i3d_track_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io, i3d_track_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!pose6_io) return fail(f, I3D_ERR_INVALID_ARGUMENT, "i3d_fusion_track: null pose");
    if (d && d->use_context_camera != 0)
        return fail(f, I3D_ERR_INVALID_ARGUMENT, "i3d_fusion_track: desc->use_context_camera must be 0 (give the depth camera's intrinsics4 / distortion5)");
    return track_frame_run(FusionModel(f, "i3d_fusion_track"), d, w, h, depth, pose6_io, stats);
}

int i3d_fusion_query_points(i3d_fusion* f, const i3d_query_desc* d, int64_t n, const double* points, double* sdf, float* normal, double* foot, double* distance,
                            uint8_t* status, i3d_query_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    return query_run(FusionModel(f, "i3d_fusion_query_points"), d, n, points, sdf, normal, nullptr, foot, distance, status, stats);
}

int i3d_fusion_cast_rays(i3d_fusion* f, int32_t order, int64_t n, const double* origins, const double* directions, const double* t_min, const double* t_max,
                         double* t, double* position, float* normal, uint8_t* status, i3d_render_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    return cast_rays_run(FusionModel(f, "i3d_fusion_cast_rays"), false, order, n, origins, directions, t_min, t_max, t, position, normal, nullptr, nullptr, nullptr, status, stats);
}

int i3d_fusion_cast_rays_color(i3d_fusion* f, int32_t order, int64_t n, const double* origins, const double* directions, const double* t_min, const double* t_max,
                               double* t, float* color, uint8_t* status, i3d_render_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    return cast_rays_run(FusionModel(f, "i3d_fusion_cast_rays_color"), false, order, n, origins, directions, t_min, t_max, t, nullptr, nullptr, nullptr, nullptr, nullptr, status,
                         stats, true, color);
}

int i3d_fusion_register_points(i3d_fusion* f, const i3d_register_desc* d, int64_t n, const double* points, double* pose6_io, i3d_register_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    return register_run(FusionModel(f, "i3d_fusion_register_points"), d, n, points, pose6_io, stats);
}

// ---- depth frames on the field, with the photometric term on the volume's fused colour (section 22) ----------------------------------
int i3d_fusion_track_sdf(i3d_fusion* f, const i3d_track_sdf_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io, i3d_track_sdf_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (d && d->use_context_camera != 0)
        return fail(f, I3D_ERR_INVALID_ARGUMENT, "i3d_fusion_track_sdf: desc->use_context_camera must be 0 (give the depth camera's intrinsics4 / distortion5)");
    return track_sdf_run(FusionModel(f, "i3d_fusion_track_sdf"), d, w, h, depth, pose6_io, stats);
}

int i3d_fusion_track_sdf_rgbd(i3d_fusion* f, const i3d_track_sdf_rgbd_desc* d, int32_t w, int32_t h, const float* depth, const float* luminance, double* pose6_io,
                              i3d_track_sdf_rgbd_stats* stats) {
    const char* fn = "i3d_fusion_track_sdf_rgbd";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!d) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null descriptor");
    if (d->base.use_context_camera != 0)
        return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": desc->base.use_context_camera must be 0 (give the depth camera's intrinsics4 / distortion5)");
    const TrackSdfRgbd r = rgbd_of(d, stats);
    return track_sdf_run(FusionModel(f, fn), &d->base, w, h, depth, pose6_io, nullptr, &r, luminance);
}

int i3d_fusion_debug_track_sdf_rgbd_sums(i3d_fusion* f, const i3d_track_sdf_rgbd_desc* d, int32_t w, int32_t h, const float* depth, const float* luminance,
                                         const double* pose6, const double* pivot3, double* sums31, int64_t* valid, int64_t* photo_samples) {
    const char* fn = "i3d_fusion_debug_track_sdf_rgbd_sums";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!d || !pose6 || !pivot3 || !sums31) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null argument");
    if (d->base.use_context_camera != 0) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": desc->base.use_context_camera must be 0");
    double pose[6];
    for (int k = 0; k < 6; ++k) pose[k] = pose6[k];
    const TrackSdfRgbd r = rgbd_of(d, nullptr);
    const TrackSdfDebug dbg{pivot3, sums31, valid, nullptr, photo_samples};
    return track_sdf_run(FusionModel(f, fn), &d->base, w, h, depth, pose, nullptr, &r, luminance, &dbg);
}

int i3d_fusion_debug_voxel_luminance(i3d_fusion* f, int64_t n, const int32_t* keys, double* c) {
    const char* fn = "i3d_fusion_debug_voxel_luminance";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!keys || !c))) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad arguments");
    if (n == 0) return I3D_OK;
    const FusionModel m(f, fn);
    if (int rc = m.make_current()) return rc;
    const double* vol = nullptr;
    if (int rc = m.fill_intensity(vol)) return rc;
    DevBuf<int> d_keys; DevBuf<double> d_out;
    F_HIP(f, d_keys.alloc(3 * (size_t)n)); F_HIP(f, d_out.alloc((size_t)n));
    F_HIP(f, hipMemcpyAsync(d_keys.p, keys, 3 * (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
    launch_fusion_luminance_lookup(f->stream, f->table(), vol, (long long)n, d_keys.p, d_out.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(c, d_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    F_HIP(f, hipStreamSynchronize(f->stream));
    return I3D_OK;
}

// SparseVoxelGrid<Voxel>::save of the finished volume, or of the open volume's last snapshot (sparse_voxel_grid.cpp:484-520)
int i3d_fusion_save(const i3d_fusion* f, const char* path) {
    if (!f || !path) return I3D_ERR_INVALID_ARGUMENT;
    if (!(f->finished || f->have_snapshot)) return I3D_ERR_STATE;
    return i3d_tsdf_write(path, f->voxel_size, f->truncation, f->weight_sample, 0.6f, f->out_sdf.size(), f->out_keys.data(), f->out_sdf.data(), f->out_weight.data(),
                          f->out_color.data());
}

int i3d_fusion_debug_poke_voxels(i3d_fusion* f, int64_t n, const int32_t* keys, const float* sdf, const float* weight, const uint8_t* color, uint8_t* found) {
    const char* fn = "i3d_fusion_debug_poke_voxels";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (n < 0 || n > (1ll << 28) || (n > 0 && (!keys || !sdf || !weight || !color || !found))) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad arguments");
    if (n == 0) return I3D_OK;
    F_HIP(f, hipSetDevice(f->device));
    hipStream_t st = f->stream;
    const size_t m = (size_t)n;
    DevBuf<int> d_keys; DevBuf<uint8_t> d_found, d_rgb; DevBuf<float> d_sdf, d_w;
    F_HIP(f, d_keys.alloc(3 * m)); F_HIP(f, d_found.alloc(m)); F_HIP(f, d_rgb.alloc(3 * m)); F_HIP(f, d_sdf.alloc(m)); F_HIP(f, d_w.alloc(m));
    F_HIP(f, hipMemcpyAsync(d_keys.p, keys, 3 * m * sizeof(int32_t), hipMemcpyHostToDevice, st));
    F_HIP(f, hipMemcpyAsync(d_sdf.p, sdf, m * sizeof(float), hipMemcpyHostToDevice, st));
    F_HIP(f, hipMemcpyAsync(d_w.p, weight, m * sizeof(float), hipMemcpyHostToDevice, st));
    F_HIP(f, hipMemcpyAsync(d_rgb.p, color, 3 * m, hipMemcpyHostToDevice, st));
    f->model.bricks.ok = false;                                         // the set of slots with weight != 0 may change
    launch_fusion_debug_poke_voxels(st, f->table(), (long long)n, d_keys.p, d_sdf.p, d_w.p, d_rgb.p, d_found.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(found, d_found.p, m, hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    return I3D_OK;
}

}  // extern "C"
