// TSDF fusion on the device — AppFusion::fuseSDF's volume (apps/src/app_fusion.cpp:107-200) behind a C handle.
//   i3d_fusion_integrate = erodeDiscontinuities + computeNormals + SparseVoxelGrid<Voxel>::integrate (alloc + update) for one frame
//   i3d_fusion_finish    = SDFAlgorithms::correctSDF + clearInvalidVoxels, and the reference's record order
//   i3d_fusion_merge     = a whole volume as one sample of the running mean under a rigid motion (none in the reference)
//   i3d_fusion_register_volume = the rigid motion that merge takes, found on the two stored fields (none in the reference)
//   i3d_fusion_extract_mesh = marching cubes over the table as it stands, welded and cleaned on the device
// Frames are integrated in call order, one allocation launch and one integration launch per frame (fusion_kernels.hip).  The saved
// volume's record order is the iteration order of the reference's unordered_map; it is reproduced from the order of first insertion
// (a per-voxel rank kept by the allocation kernel, radix-sorted here) by replaying the insertions epoch by epoch on the device (map_order.hip) — the same replay levels.cpp uses for the level
// transitions.
#include "../../../include/intrinsic3d_hip.h"
#include "../device/fusion_kernels.hpp"
#include "../device/register_volume_kernels.hpp"
#include "../device/fusion_mesh_kernels.hpp"
#include "../device/frame_math.hpp"
#include "context.hpp"
#include "map_order.hpp"
#include "mesh_internal.hpp"
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <unordered_map>
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

struct i3d_fusion {
    int device = 0; hipStream_t stream = nullptr;
    float voxel_size = 0, truncation = 0, depth_min = 0, depth_max = 0, weight_sample = 10.0f;      // sparse_voxel_grid.cpp:44-51
    float clip[6] = {0, 0, 0, 0, 0, 0}; bool use_clip = false;
    unsigned long long capacity = 0, frames = 0;      // frames: integrate operations so far = the next ordinal (it feeds the rank and is never decremented)
    std::vector<bool> live;                           // per ordinal: the frame is in the volume (integrate marks, deintegrate / reintegrate clear)
    DevBuf<unsigned long long> keys, rank, crank; DevBuf<float> sdf, weight; DevBuf<uchar4> color;
    DevBuf<unsigned long long> d_count; DevBuf<int> d_flag;
    DevBuf<float> d_depth_raw, d_depth, d_normals; DevBuf<uint8_t> d_bgr;
    // result of finish()
    bool finished = false, corrected = false;      // corrected: correctSDF has been written into the table (finish is not re-runnable past that point)
    std::vector<int32_t> out_keys; std::vector<float> out_sdf, out_weight; std::vector<uint8_t> out_color;
    unsigned long long allocated = 0; int correct_launches = 0;
    // the volume as a model (i3d_fusion_render / i3d_fusion_track): brick bitmap of the slots with weight != 0, cached until integrate / finish
    // change the table (positional: a growth alone keeps it); output planes, stats and the tracking buffers, grown only
    DevBuf<unsigned> render_bits; DevBuf<int> render_bounds; int render_lo[3] = {0, 0, 0}, render_dim[3] = {0, 0, 0}; bool render_bricks_ok = false;
    DevBuf<float> render_planes; DevBuf<RenderStatsDev> render_stats;
    TrackBuffers track;
    DevBuf<unsigned char> query_scratch;      // point queries (query.cpp's driver): the one scratch of a call, grown only
    DevBuf<unsigned char> register_scratch;   // point-set registration (register.cpp's driver): the one scratch of a call, grown only
    // volume-to-volume registration, in the handle of the volume registered against: flags | scan | list | sorted list | scan / sort temp | slab | state
    DevBuf<unsigned char> register_volume_scratch; size_t register_volume_entries = 0, register_volume_temp = 0;      // what the last call's layout held
    TrackSdfBuffers track_sdf;                // depth frames on the field (track_sdf.cpp's driver): its buffers, grown only
    // the luminance of the fused colour per table slot (i3d_fusion_track_sdf_rgbd): [capacity], grown only, filled anew by every call that has a
    // photometric weight and read by that call alone (integrate, finish and a growth of the table move or change slots)
    DevBuf<double> track_sdf_luminance;
    // i3d_fusion_merge: its two counts and the buffers of the rank finalisation, grown only
    DevBuf<unsigned long long> merge_counts, merge_key0, merge_key1; DevBuf<int> merge_flags, merge_offs; DevBuf<unsigned int> merge_slot0, merge_slot1; DevBuf<char> merge_tmp;
    // i3d_fusion_extract_mesh: per-slot and per-list-entry scratch and the device mesh, grown only; the triangle table, uploaded once; the last mesh
    DevBuf<unsigned char> mesh_slots, mesh_list, mesh_out; DevBuf<unsigned char> mesh_ntri; DevBuf<signed char> mesh_tri; bool mesh_tables_ok = false;
    MeshData mesh; bool have_mesh = false;
    std::string error;
    FusionTable table() { return FusionTable{keys.p, sdf.p, weight.p, color.p, rank.p, crank.p, capacity - 1}; }
};

namespace {

int fail(i3d_fusion* f, int code, const std::string& msg) { if (f) f->error = msg; return code; }
#define F_HIP(f, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(f, I3D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

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

// the brick bitmap of the table as it stands (DESIGN.md 13.1 item 3 over the slots with weight != 0)
int fusion_ensure_bricks(i3d_fusion* f) {
    if (f->render_bricks_ok) return I3D_OK;
    hipStream_t st = f->stream;
    const int init[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
    int b[6];
    F_HIP(f, f->render_bounds.alloc(6));
    F_HIP(f, hipMemcpyAsync(f->render_bounds.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    launch_fusion_brick_bounds(st, f->table(), f->render_bounds.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(b, f->render_bounds.p, sizeof(b), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    for (int a = 0; a < 3; ++a) { f->render_lo[a] = 0; f->render_dim[a] = 0; }
    if (b[0] <= b[3]) {                          // else nothing has a weight: the box is empty and every ray misses
        long long bits = 1;
        for (int a = 0; a < 3; ++a) { f->render_lo[a] = b[a]; f->render_dim[a] = b[3 + a] - b[a] + 1; bits *= f->render_dim[a]; }
        if (bits > (1ll << 31)) {
            for (int a = 0; a < 3; ++a) f->render_dim[a] = 0;
            return fail(f, I3D_ERR_CAPACITY, "fusion: the brick bitmap of the volume's bounding box would exceed 2^31 bits (" + std::to_string(bits) + ")");
        }
        const size_t words = (size_t)((bits + 31) / 32);
        F_HIP(f, f->render_bits.alloc(words));
        F_HIP(f, hipMemsetAsync(f->render_bits.p, 0, words * sizeof(unsigned), st));
        launch_fusion_brick_fill(st, f->table(), f->render_bits.p, f->render_lo, f->render_dim);
        F_HIP(f, hipGetLastError());
    }
    f->render_bricks_ok = true;
    return I3D_OK;
}

FusionRenderGrid fusion_grid(i3d_fusion* f) {
    return FusionRenderGrid{f->table(), (double)f->voxel_size, f->render_bits.p, {f->render_lo[0], f->render_lo[1], f->render_lo[2]},
                            {f->render_dim[0], f->render_dim[1], f->render_dim[2]}};
}

// the table as the kernels that sample the field at points read it (queries, registration): no brick bitmap, nothing marches
FusionRenderGrid field_grid(i3d_fusion* f) { return FusionRenderGrid{f->table(), (double)f->voxel_size, nullptr, {0, 0, 0}, {0, 0, 0}}; }

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
    if (f->finished || f->corrected) return fail(f, I3D_ERR_STATE, std::string(fn) + ": the volume has been finished (or a finish failed after correcting the table)");
    if (ordinal >= f->live.size() || !f->live[ordinal])
        return fail(f, I3D_ERR_STATE, std::string(fn) + ": ordinal " + std::to_string(ordinal) + " is not a frame of this volume (never integrated, or already taken out)");
    return I3D_OK;
}

constexpr int FUSION_RENDER_MAX_EDGE = 1 << 15;      // as i3d_render_view

}  // namespace

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
    if (f->finished || f->corrected) return fail(f, I3D_ERR_STATE, std::string(fn) + ": the volume has been finished (or a finish failed after correcting the table)");
    F_HIP(f, hipSetDevice(f->device));
    f->render_bricks_ok = false;                     // the weights and values change
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
    f->render_bricks_ok = false;
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
    f->render_bricks_ok = false;
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
    if (!src) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null source volume");
    if (f == src) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": a volume cannot be merged into itself");
    if (f->device != src->device) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": the volumes are on different devices");
    if (std::memcmp(&f->voxel_size, &src->voxel_size, sizeof(float)) != 0 || std::memcmp(&f->truncation, &src->truncation, sizeof(float)) != 0)
        return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": the volumes must have the same voxel size and truncation, bit for bit");
    for (int k = 0; pose6 && k < 6; ++k)
        if (!std::isfinite(pose6[k])) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": the pose is not finite");
    if (f->finished || f->corrected) return fail(f, I3D_ERR_STATE, fn + ": the volume has been finished (or a finish failed after correcting the table)");

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
    if (int rc = fusion_ensure_bricks(src)) return fail(f, rc, fn + ": the source volume: " + src->error);
    F_HIP(f, hipStreamSynchronize(src->stream));                         // src is read on f's stream from here on
    i3d_merge_stats out; std::memset(&out, 0, sizeof(out));
    out.ordinal = f->frames; out.aligned = aligned ? 1 : 0;
    for (int i = 0; i < 9; ++i) out.rotation[i] = mg.R[i];
    for (int a = 0; a < 3; ++a) out.translation_voxels[a] = mg.tv[a];
    if (src->render_dim[0] > 0) {                                        // else nothing in src has a weight: no launch, the table is untouched
        hipStream_t st = f->stream;
        for (int a = 0; a < 3; ++a) { mg.lo[a] = src->render_lo[a] * (1 << RENDER_BRICK_SHIFT); mg.hi[a] = (src->render_lo[a] + src->render_dim[a]) * (1 << RENDER_BRICK_SHIFT); }
        f->render_bricks_ok = false;                                     // voxels appear, weights and values change
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
        const size_t n = (size_t)(after - before), cap = (size_t)f->capacity;
        if (n > 0) {                                                     // the final ranks: position among the inserted voxels in ascending order of packed key
            FusionTable t = f->table(); size_t bytes = 0;
            F_HIP(f, f->merge_flags.alloc(cap)); F_HIP(f, f->merge_offs.alloc(cap));
            F_HIP(f, f->merge_key0.alloc(n)); F_HIP(f, f->merge_key1.alloc(n)); F_HIP(f, f->merge_slot0.alloc(n)); F_HIP(f, f->merge_slot1.alloc(n));
            launch_fusion_merge_flag(st, t, mg.ordinal, f->merge_flags.p);
            F_HIP(f, rocprim::exclusive_scan(nullptr, bytes, f->merge_flags.p, f->merge_offs.p, 0, cap, rocprim::plus<int>(), st));
            F_HIP(f, f->merge_tmp.alloc(bytes));
            F_HIP(f, rocprim::exclusive_scan(f->merge_tmp.p, bytes, f->merge_flags.p, f->merge_offs.p, 0, cap, rocprim::plus<int>(), st));
            launch_fusion_merge_gather(st, t, f->merge_flags.p, f->merge_offs.p, (long long)n, f->merge_key0.p, f->merge_slot0.p);
            bytes = 0;
            F_HIP(f, rocprim::radix_sort_pairs(nullptr, bytes, f->merge_key0.p, f->merge_key1.p, f->merge_slot0.p, f->merge_slot1.p, n, 0, 64, st));
            F_HIP(f, f->merge_tmp.alloc(bytes));
            F_HIP(f, rocprim::radix_sort_pairs(f->merge_tmp.p, bytes, f->merge_key0.p, f->merge_key1.p, f->merge_slot0.p, f->merge_slot1.p, n, 0, 64, st));
            launch_fusion_merge_rank(st, t, mg.ordinal, (long long)n, f->merge_slot1.p);
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
    f->render_bricks_ok = false;                     // correctSDF writes values and weights
    hipStream_t st = f->stream; FusionTable t = f->table();
    const unsigned long long cap = f->capacity;
    // 1. occupied slots, sorted by first-insertion rank = the reference's insertion sequence
    DevBuf<int> flags, offs; DevBuf<char> tmp; size_t bytes = 0;
    F_HIP(f, flags.alloc(cap)); F_HIP(f, offs.alloc(cap));
    launch_fusion_occupied(st, t, flags.p);
    F_HIP(f, rocprim::exclusive_scan(nullptr, bytes, flags.p, offs.p, 0, (size_t)cap, rocprim::plus<int>(), st));
    F_HIP(f, tmp.alloc(bytes));
    F_HIP(f, rocprim::exclusive_scan(tmp.p, bytes, flags.p, offs.p, 0, (size_t)cap, rocprim::plus<int>(), st));
    unsigned long long m = 0;
    F_HIP(f, hipMemcpyAsync(&m, f->d_count.p, sizeof(m), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    f->allocated = m;
    if (m > 0x7FFFFFFFull) return fail(f, I3D_ERR_CAPACITY, "fusion: more than 2^31 voxels");
    f->out_keys.clear(); f->out_sdf.clear(); f->out_weight.clear(); f->out_color.clear();
    if (m == 0) { f->finished = true; if (count) *count = 0; return I3D_OK; }
    DevBuf<unsigned long long> rank0, rank1; DevBuf<unsigned int> slot0, slot1;
    F_HIP(f, rank0.alloc(m)); F_HIP(f, rank1.alloc(m)); F_HIP(f, slot0.alloc(m)); F_HIP(f, slot1.alloc(m));
    launch_fusion_gather_rank(st, t, flags.p, offs.p, rank0.p, slot0.p);
    bytes = 0;
    F_HIP(f, rocprim::radix_sort_pairs(nullptr, bytes, rank0.p, rank1.p, slot0.p, slot1.p, (size_t)m, 0, 64, st));
    F_HIP(f, tmp.alloc(bytes));
    F_HIP(f, rocprim::radix_sort_pairs(tmp.p, bytes, rank0.p, rank1.p, slot0.p, slot1.p, (size_t)m, 0, 64, st));
    // 2. replay the insertions: iteration order of the reference's map
    DevBuf<int> kxyz; F_HIP(f, kxyz.alloc(3 * m));
    launch_fusion_keys(st, t, (long long)m, slot1.p, kxyz.p);
    DevBuf<int> d_order, pos_of_slot; DevBuf<unsigned int> visit_slot;
    F_HIP(f, d_order.alloc(m)); F_HIP(f, pos_of_slot.alloc(cap)); F_HIP(f, visit_slot.alloc(m));
    { const std::vector<MapEpoch> ep = map_epochs((size_t)m);                                            // keys of a hash table: distinct by construction
      F_HIP(f, map_order_device(st, kxyz.p, (size_t)m, ep.data(), (int)ep.size(), d_order.p)); }
    launch_fusion_positions(st, (long long)m, slot1.p, d_order.p, visit_slot.p, pos_of_slot.p);
    // 3. correctSDF: up to `correct_iterations` in-place sweeps, each evaluated as a fixed point (see k_correct), in a spatially sorted
    //    compact index space with the 26 neighbour indices resolved once
    if (correct_iterations > 0) {
        DevBuf<unsigned long long> sk0, sk1; DevBuf<unsigned int> slot_c; DevBuf<int> compact_of_slot, c_pos, nbr; DevBuf<float> c_sdf, c_cur;
        DevBuf<unsigned char> c_valid, c_touched, c_upd;
        F_HIP(f, sk0.alloc(m)); F_HIP(f, sk1.alloc(m)); F_HIP(f, slot_c.alloc(m)); F_HIP(f, compact_of_slot.alloc(cap)); F_HIP(f, c_pos.alloc(m));
        F_HIP(f, nbr.alloc(26 * m)); F_HIP(f, c_sdf.alloc(m)); F_HIP(f, c_cur.alloc(m)); F_HIP(f, c_valid.alloc(m)); F_HIP(f, c_touched.alloc(m)); F_HIP(f, c_upd.alloc(m));
        launch_fusion_spatial_keys(st, t, (long long)m, slot1.p, sk0.p);
        bytes = 0;
        F_HIP(f, rocprim::radix_sort_pairs(nullptr, bytes, sk0.p, sk1.p, slot1.p, slot_c.p, (size_t)m, 0, 64, st));
        F_HIP(f, tmp.alloc(bytes));
        F_HIP(f, rocprim::radix_sort_pairs(tmp.p, bytes, sk0.p, sk1.p, slot1.p, slot_c.p, (size_t)m, 0, 64, st));
        launch_fusion_compact_init(st, t, (long long)m, slot_c.p, pos_of_slot.p, compact_of_slot.p, c_sdf.p, c_pos.p, c_valid.p, c_touched.p);
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
    DevBuf<int> vflags, voffs;
    F_HIP(f, vflags.alloc(m)); F_HIP(f, voffs.alloc(m));
    launch_fusion_valid(st, t, (long long)m, visit_slot.p, vflags.p);
    bytes = 0;
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
        launch_fusion_export(st, t, (long long)m, visit_slot.p, vflags.p, voffs.p, ok.p, os.p, ow.p, oc.p);
        f->out_keys.resize(3 * nv); f->out_sdf.resize(nv); f->out_weight.resize(nv); f->out_color.resize(3 * nv);
        F_HIP(f, hipMemcpyAsync(f->out_keys.data(), ok.p, sizeof(int) * 3 * nv, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipMemcpyAsync(f->out_sdf.data(), os.p, sizeof(float) * nv, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipMemcpyAsync(f->out_weight.data(), ow.p, sizeof(float) * nv, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipMemcpyAsync(f->out_color.data(), oc.p, 3 * nv, hipMemcpyDeviceToHost, st));
        F_HIP(f, hipStreamSynchronize(st));
    }
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
    if (!f || !f->finished) return I3D_ERR_STATE;
    const size_t n = f->out_sdf.size();
    if (keys) std::memcpy(keys, f->out_keys.data(), sizeof(int32_t) * 3 * n);
    if (sdf) std::memcpy(sdf, f->out_sdf.data(), sizeof(float) * n);
    if (weight) std::memcpy(weight, f->out_weight.data(), sizeof(float) * n);
    if (color) std::memcpy(color, f->out_color.data(), 3 * n);
    return I3D_OK;
}

int i3d_fusion_render(i3d_fusion* f, const i3d_render_desc* d, float* depth, float* normal, i3d_render_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!d) return fail(f, I3D_ERR_INVALID_ARGUMENT, "i3d_fusion_render: null descriptor");
    if (d->frame != -1) return fail(f, I3D_ERR_INVALID_ARGUMENT, "i3d_fusion_render: desc->frame must be -1 (a free camera; the volume has no keyframes)");
    if (d->width <= 0 || d->height <= 0 || d->width > FUSION_RENDER_MAX_EDGE || d->height > FUSION_RENDER_MAX_EDGE)
        return fail(f, I3D_ERR_INVALID_ARGUMENT, "i3d_fusion_render: image size (desc->width / height) out of range");
    const RenderCam cam = render_cam(camera_of(d->intrinsics4, d->distortion5, d->width, d->height), d->pose6, d->min_depth, d->max_depth);
    F_HIP(f, hipSetDevice(f->device));
    if (int rc = fusion_ensure_bricks(f)) return rc;
    hipStream_t st = f->stream;
    const size_t px = (size_t)d->width * d->height;
    if (depth || normal) F_HIP(f, f->render_planes.alloc(4 * px));
    F_HIP(f, f->render_stats.alloc(1));
    float* base = f->render_planes.p;
    const RenderPlanes out{depth ? base : nullptr, normal ? base + px : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    F_HIP(f, hipMemsetAsync(f->render_stats.p, 0, sizeof(RenderStatsDev), st));
    launch_render(st, fusion_grid(f), cam, out, f->render_stats.p);
    F_HIP(f, hipGetLastError());
    if (depth) F_HIP(f, hipMemcpyAsync(depth, out.depth, px * sizeof(float), hipMemcpyDeviceToHost, st));
    if (normal) F_HIP(f, hipMemcpyAsync(normal, out.normal, 3 * px * sizeof(float), hipMemcpyDeviceToHost, st));
    RenderStatsDev s{};
    F_HIP(f, hipMemcpyAsync(&s, f->render_stats.p, sizeof(s), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    if (stats) { stats->hits = (int64_t)s.hits; stats->samples = (int64_t)s.samples; stats->residual_sq_sum = 0.0; }
    return I3D_OK;
}

int i3d_fusion_track(i3d_fusion* f, const i3d_track_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io, i3d_track_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!pose6_io) return fail(f, I3D_ERR_INVALID_ARGUMENT, "i3d_fusion_track: null pose");
    if (d && d->use_context_camera != 0)
        return fail(f, I3D_ERR_INVALID_ARGUMENT, "i3d_fusion_track: desc->use_context_camera must be 0 (give the depth camera's intrinsics4 / distortion5)");
    TrackModel m;
    m.fail = [f](int code, const std::string& msg) { return fail(f, code, msg); };
    m.ready = [f](const i3d_track_desc&, const double*&, const double*&) -> int {
        F_HIP(f, hipSetDevice(f->device));
        return fusion_ensure_bricks(f);
    };
    m.cast = [f](const RenderCam& cam, const RenderPlanes& out, RenderStatsDev* s) { launch_render(f->stream, fusion_grid(f), cam, out, s); };
    return track_frame_run(f->stream, f->track, m, "i3d_fusion_track", d, w, h, depth, pose6_io, stats);
}

int i3d_fusion_query_points(i3d_fusion* f, const i3d_query_desc* d, int64_t n, const double* points, double* sdf, float* normal, double* foot, double* distance,
                            uint8_t* status, i3d_query_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    QueryModel m;
    m.fail = [f](int code, const std::string& msg) { return fail(f, code, msg); };
    m.ready = [f]() -> int { F_HIP(f, hipSetDevice(f->device)); return I3D_OK; };
    m.launch = [f](const QueryParams& p, const double* pts, const QueryOut& out, QueryRow* rows, QueryRow* total) {
        launch_query(f->stream, field_grid(f), p, pts, out, rows, total);
    };
    m.voxel_size = (double)f->voxel_size;
    return query_run(f->stream, f->query_scratch, m, "i3d_fusion_query_points", d, n, points, sdf, normal, nullptr, foot, distance, status, stats);
}

int i3d_fusion_register_points(i3d_fusion* f, const i3d_register_desc* d, int64_t n, const double* points, double* pose6_io, i3d_register_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    RegisterModel m;
    m.fail = [f](int code, const std::string& msg) { return fail(f, code, msg); };
    m.ready = [f]() -> int { F_HIP(f, hipSetDevice(f->device)); return I3D_OK; };
    m.launch = [f](const RegisterParams& p, const double* pts, const TrackState* state, int check_done, double* slab) {
        launch_register(f->stream, field_grid(f), p, pts, state, check_done, slab);
    };
    m.voxel_size = (double)f->voxel_size;
    return register_run(f->stream, f->register_scratch, m, "i3d_fusion_register_points", d, n, points, pose6_io, stats);
}

// ---- depth frames on the field, with the photometric term on the volume's fused colour (section 22) ----------------------------------
}  // extern "C"

namespace {

// the luminance volume of the table as it stands, on the handle's stream (section 22.1 item 1); no cache across calls
int fill_luminance(i3d_fusion* f, const double*& vol) {
    F_HIP(f, f->track_sdf_luminance.alloc((size_t)f->capacity));
    launch_fusion_voxel_luminance(f->stream, f->table(), f->track_sdf_luminance.p);
    vol = f->track_sdf_luminance.p;
    return I3D_OK;
}

TrackSdfModel fusion_sdf_model(i3d_fusion* f) {
    TrackSdfModel m;
    m.fail = [f](int code, const std::string& msg) { return fail(f, code, msg); };
    m.ready = [f](const i3d_track_sdf_desc&, const double*&, const double*&) -> int { F_HIP(f, hipSetDevice(f->device)); return I3D_OK; };
    m.intensity_ready = []() -> int { return I3D_OK; };      // the colour is always there: no SH is involved
    m.intensity = [f](const double*& vol) -> int { return fill_luminance(f, vol); };
    m.launch = [f](const TrackSdfParams& p, const TrackSdfPhoto* ph, const TrackSdfBatch& b, int check_done) {
        launch_track_sdf(f->stream, field_grid(f), p, ph, b, check_done);
    };
    m.voxel_size = (double)f->voxel_size;
    return m;
}

TrackSdfRgbd rgbd_of(const i3d_track_sdf_rgbd_desc* d, i3d_track_sdf_rgbd_stats* stats) {
    TrackSdfRgbd r; r.geometric_weight = d->geometric_weight; r.photo_weight = d->photo_weight; r.max_photo_residual = d->max_photo_residual; r.stats = stats;
    return r;
}

}  // namespace

extern "C" {

int i3d_fusion_track_sdf(i3d_fusion* f, const i3d_track_sdf_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io, i3d_track_sdf_stats* stats) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (d && d->use_context_camera != 0)
        return fail(f, I3D_ERR_INVALID_ARGUMENT, "i3d_fusion_track_sdf: desc->use_context_camera must be 0 (give the depth camera's intrinsics4 / distortion5)");
    return track_sdf_run(f->stream, f->track_sdf, fusion_sdf_model(f), "i3d_fusion_track_sdf", d, w, h, depth, pose6_io, stats);
}

int i3d_fusion_track_sdf_rgbd(i3d_fusion* f, const i3d_track_sdf_rgbd_desc* d, int32_t w, int32_t h, const float* depth, const float* luminance, double* pose6_io,
                              i3d_track_sdf_rgbd_stats* stats) {
    const char* fn = "i3d_fusion_track_sdf_rgbd";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!d) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null descriptor");
    if (d->base.use_context_camera != 0)
        return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": desc->base.use_context_camera must be 0 (give the depth camera's intrinsics4 / distortion5)");
    const TrackSdfRgbd r = rgbd_of(d, stats);
    return track_sdf_run(f->stream, f->track_sdf, fusion_sdf_model(f), fn, &d->base, w, h, depth, pose6_io, nullptr, &r, luminance);
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
    return track_sdf_run(f->stream, f->track_sdf, fusion_sdf_model(f), fn, &d->base, w, h, depth, pose, nullptr, &r, luminance, &dbg);
}

int i3d_fusion_debug_voxel_luminance(i3d_fusion* f, int64_t n, const int32_t* keys, double* c) {
    const char* fn = "i3d_fusion_debug_voxel_luminance";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (n < 0 || (n > 0 && (!keys || !c))) return fail(f, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad arguments");
    if (n == 0) return I3D_OK;
    F_HIP(f, hipSetDevice(f->device));
    const double* vol = nullptr;
    if (int rc = fill_luminance(f, vol)) return rc;
    DevBuf<int> d_keys; DevBuf<double> d_out;
    F_HIP(f, d_keys.alloc(3 * (size_t)n)); F_HIP(f, d_out.alloc((size_t)n));
    F_HIP(f, hipMemcpyAsync(d_keys.p, keys, 3 * (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, f->stream));
    launch_fusion_luminance_lookup(f->stream, f->table(), vol, (long long)n, d_keys.p, d_out.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(c, d_out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    F_HIP(f, hipStreamSynchronize(f->stream));
    return I3D_OK;
}

// SparseVoxelGrid<Voxel>::save of the finished volume (sparse_voxel_grid.cpp:484-520)
int i3d_fusion_save(const i3d_fusion* f, const char* path) {
    if (!f || !path) return I3D_ERR_INVALID_ARGUMENT;
    if (!f->finished) return I3D_ERR_STATE;
    return i3d_tsdf_write(path, f->voxel_size, f->truncation, f->weight_sample, 0.6f, f->out_sdf.size(), f->out_keys.data(), f->out_sdf.data(), f->out_weight.data(),
                          f->out_color.data());
}

}  // extern "C"

// ---- one volume aligned to another on the two stored fields ----------------------------------------------------------------------------
namespace {

constexpr long long REGISTER_VOLUME_MAX = 1ll << 27;
constexpr int REGISTER_VOLUME_MAX_ITERATIONS = 200, REGISTER_VOLUME_MAX_STRIDE = 64;

// the sorted list of src's selected voxels and the buffers of the loop, all inside the owner's register_volume_scratch
struct VolumePass { VolumeList list; double* slab; TrackState* state; };
struct VolumeDebug { const double* pivot3; int64_t limit; int32_t row_cap; double* sums29; int64_t* valid; int64_t* selected; };

int volume_desc_check(i3d_fusion* owner, const std::string& fn, const i3d_register_volume_desc* d) {
    if (!d) return fail(owner, I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (d->iterations < 0 || d->iterations > REGISTER_VOLUME_MAX_ITERATIONS)
        return fail(owner, I3D_ERR_INVALID_ARGUMENT, fn + ": iterations must be 0.." + std::to_string(REGISTER_VOLUME_MAX_ITERATIONS));
    if (d->stride < 1 || d->stride > REGISTER_VOLUME_MAX_STRIDE)
        return fail(owner, I3D_ERR_INVALID_ARGUMENT, fn + ": stride must be 1.." + std::to_string(REGISTER_VOLUME_MAX_STRIDE));
    if (!std::isfinite(d->source_band_voxels) || !(d->source_band_voxels > 0.0))
        return fail(owner, I3D_ERR_INVALID_ARGUMENT, fn + ": source_band_voxels must be finite and > 0");
    if (!std::isfinite(d->max_distance) || !(d->max_distance > 0.0)) return fail(owner, I3D_ERR_INVALID_ARGUMENT, fn + ": max_distance must be finite and > 0");
    return I3D_OK;
}

// Section 28.1 items 2 and 3 on owner's stream: flag, scan, gather, sort by packed key.  One synchronisation, for the count; a second round of flag and scan only
// when the scratch has to grow for it (the growth drops the flags).  owner == src for the debug entry that only lists.
int volume_select(i3d_fusion* owner, i3d_fusion* src, const std::string& fn, const i3d_register_volume_desc* d, VolumePass& out) {
    F_HIP(owner, hipSetDevice(owner->device));
    if (owner != src) F_HIP(owner, hipStreamSynchronize(src->stream));          // src is read on owner's stream from here on
    hipStream_t st = owner->stream;
    const size_t cap = (size_t)src->capacity;
    const VolumeSelect sel{d->source_band_voxels * (double)src->voxel_size, d->stride};
    size_t scan_bytes = 0;
    F_HIP(owner, rocprim::exclusive_scan(nullptr, scan_bytes, (int*)nullptr, (int*)nullptr, 0, cap, rocprim::plus<int>(), st));
    size_t have = owner->register_volume_entries, temp = std::max(owner->register_volume_temp, scan_bytes), n = 0;
    unsigned char* base = nullptr;
    size_t o_flags = 0, o_offs = 0, o_k0 = 0, o_k1 = 0, o_s0 = 0, o_s1 = 0, o_tmp = 0, o_slab = 0, o_state = 0;
    for (;;) {
        size_t total = 0;
        auto take = [&total](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
        const size_t rows = std::min<size_t>(REGISTER_MAX_ROWS, (have + REGISTER_BLOCK - 1) / REGISTER_BLOCK);
        o_flags = take(cap * sizeof(int)); o_offs = take(cap * sizeof(int));
        o_k0 = take(have * sizeof(unsigned long long)); o_k1 = take(have * sizeof(unsigned long long)); o_s0 = take(have * sizeof(float)); o_s1 = take(have * sizeof(float));
        o_tmp = take(temp); o_slab = take(rows * TRACK_COLS * sizeof(double)); o_state = take(sizeof(TrackState));
        F_HIP(owner, owner->register_volume_scratch.alloc(total));
        owner->register_volume_entries = have; owner->register_volume_temp = temp;
        base = owner->register_volume_scratch.p;
        int* flags = (int*)(base + o_flags); int* offs = (int*)(base + o_offs);
        launch_volume_select_flag(st, src->table(), sel, flags);
        F_HIP(owner, hipGetLastError());
        size_t bytes = temp;
        F_HIP(owner, rocprim::exclusive_scan(base + o_tmp, bytes, flags, offs, 0, cap, rocprim::plus<int>(), st));
        int last[2] = {0, 0};
        F_HIP(owner, hipMemcpyAsync(&last[0], flags + (cap - 1), sizeof(int), hipMemcpyDeviceToHost, st));
        F_HIP(owner, hipMemcpyAsync(&last[1], offs + (cap - 1), sizeof(int), hipMemcpyDeviceToHost, st));
        F_HIP(owner, hipStreamSynchronize(st));
        n = (size_t)last[0] + (size_t)last[1];
        if ((long long)n > REGISTER_VOLUME_MAX)
            return fail(owner, I3D_ERR_CAPACITY, fn + ": " + std::to_string(n) + " voxels selected, more than 2^27: raise stride (now " + std::to_string(d->stride) +
                                                     ") or lower source_band_voxels");
        size_t sort_bytes = 0;
        if (n > 0) F_HIP(owner, rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (float*)nullptr,
                                                          (float*)nullptr, n, 0, 64, st));
        if (n <= have && sort_bytes <= temp) break;
        have = std::max(have, n); temp = std::max(temp, sort_bytes);
    }
    unsigned long long* k0 = (unsigned long long*)(base + o_k0); unsigned long long* k1 = (unsigned long long*)(base + o_k1);
    float* s0 = (float*)(base + o_s0); float* s1 = (float*)(base + o_s1);
    if (n > 0) {
        launch_volume_select_gather(st, src->table(), (const int*)(base + o_flags), (const int*)(base + o_offs), (long long)n, k0, s0);
        F_HIP(owner, hipGetLastError());
        size_t bytes = temp;
        F_HIP(owner, rocprim::radix_sort_pairs(base + o_tmp, bytes, k0, k1, s0, s1, n, 0, 64, st));
    }
    out.list = VolumeList{k1, s1, (long long)n, (double)src->voxel_size};
    out.slab = (double*)(base + o_slab); out.state = (TrackState*)(base + o_state);
    return I3D_OK;
}

// validation, the selection, the pivot, the whole budget launched back to back, the figures at the returned pose (register.cpp's loop over the list); three
// synchronisations: the count, the pivot, the result.  dbg: one pass at pose6_io about the given pivot over the first `limit` entries
int register_volume_run(i3d_fusion* f, i3d_fusion* src, const std::string& fn, const i3d_register_volume_desc* d, double* pose6_io, i3d_register_volume_stats* stats,
                        const VolumeDebug* dbg) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!src) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null source volume");
    if (int rc = volume_desc_check(f, fn, d)) return rc;
    if (!pose6_io) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null pose");
    if (f == src) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": a volume cannot be registered to itself");
    if (f->device != src->device) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": the volumes are on different devices");
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(pose6_io[k])) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": the pose is not finite");
    if (dbg && (dbg->limit < 0 || dbg->row_cap < 0 || dbg->row_cap > REGISTER_MAX_ROWS))
        return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": limit must be >= 0 and row_cap 0..8192 (0: all / the default)");

    VolumePass vp;
    if (int rc = volume_select(f, src, fn, d, vp)) return rc;
    hipStream_t st = f->stream;
    i3d_register_volume_stats out; std::memset(&out, 0, sizeof(out));
    out.status = 2; out.selected = (int64_t)vp.list.n;
    if (dbg) {
        if (dbg->sums29) std::memset(dbg->sums29, 0, TRACK_SUMS * sizeof(double));
        if (dbg->valid) *dbg->valid = 0;
        if (dbg->selected) *dbg->selected = out.selected;
    }
    const long long n = dbg && dbg->limit > 0 && dbg->limit < vp.list.n ? (long long)dbg->limit : vp.list.n;
    if (n == 0) { if (stats) *stats = out; return I3D_OK; }      // an empty src, or nothing selected: status 2 without a sums launch

    const int row_cap = dbg && dbg->row_cap > 0 ? dbg->row_cap : REGISTER_MAX_ROWS;
    const int P = register_per_lane(n, row_cap), rows = register_rows(n, P);
    const FusionRenderGrid g = field_grid(f);
    FrameConst fc; fm::frame_from_pose(pose6_io, fc);            // x_f = R x_src + t
    const double* R0 = fc.hot.R; const double* t0 = pose6_io + 3;
    TrackState hs; std::memset(&hs, 0, sizeof(hs));
    RegisterParams prm; prm.n = n; prm.per_lane = P; prm.max_distance = d->max_distance;
    if (dbg) {
        for (int a = 0; a < 3; ++a) prm.c[a] = dbg->pivot3[a];
    } else {                                                     // the pivot: c = R0 mean(p) + t0 over the list's points that count, fixed for the call
        launch_register_volume_mean(st, vp.list, P, R0, t0, g.vs, vp.slab);
        launch_track_solve(st, vp.state, vp.slab, 1, rows, 1, 28, 0.0, 0.0);
        F_HIP(f, hipGetLastError());
        F_HIP(f, hipMemcpyAsync(&hs, vp.state, sizeof(hs), hipMemcpyDeviceToHost, st));
        F_HIP(f, hipStreamSynchronize(st));
        pivot_of(hs.sums, R0, t0, prm.c);
    }
    start_state(hs, R0, t0, prm.c);
    F_HIP(f, hipMemcpyAsync(vp.state, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
    const int budget = dbg ? 0 : d->iterations;
    for (int it = 0; it < budget; ++it) {                        // back to back; once done is set the remaining launches return at once
        launch_register_volume(st, g, prm, vp.list, vp.state, 1, vp.slab);
        launch_track_solve(st, vp.state, vp.slab, 1, rows, 0, 28, d->stop_rotation, d->stop_translation);
    }
    launch_register_volume(st, g, prm, vp.list, vp.state, 0, vp.slab);      // the figures at the returned pose: totals only
    launch_track_solve(st, vp.state, vp.slab, 1, rows, 1, 28, 0.0, 0.0);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(&hs, vp.state, sizeof(hs), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    if (dbg) {
        if (dbg->sums29) for (int k = 0; k < TRACK_SUMS; ++k) dbg->sums29[k] = hs.sums[k];
        if (dbg->valid) *dbg->valid = (int64_t)hs.sums[TRACK_SUMS];
        return I3D_OK;
    }
    out.valid = (int64_t)hs.sums[TRACK_SUMS]; out.inliers = (int64_t)hs.sums[28];
    out.rms_final = rms_of(hs.sums[27], hs.sums[28]);
    out.rms_initial = budget > 0 ? hs.rms_first : out.rms_final;
    out.iterations = hs.iters;
    out.min_pivot_ratio = hs.min_pivot_ratio;
    out.status = budget > 0 ? hs.status : (out.inliers < TRACK_MIN_INLIERS ? 2 : 1);
    if (hs.iters > 0) {                                          // no step applied: the pose is left as it came in, bit for bit
        rot_to_aa(hs.R, pose6_io);
        for (int a = 0; a < 3; ++a) pose6_io[3 + a] = hs.t[a] + prm.c[a];
    }
    if (stats) *stats = out;
    return I3D_OK;
}

}  // namespace

extern "C" {

void i3d_register_volume_desc_default(i3d_register_volume_desc* d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->iterations = 30; d->stride = 1; d->source_band_voxels = 2.0; d->max_distance = 0.05; d->stop_rotation = 1e-6; d->stop_translation = 1e-6;
}

int i3d_fusion_register_volume(i3d_fusion* f, i3d_fusion* src, const i3d_register_volume_desc* desc, double* pose6_io, i3d_register_volume_stats* stats) {
    return register_volume_run(f, src, "i3d_fusion_register_volume", desc, pose6_io, stats, nullptr);
}

int i3d_fusion_debug_register_volume_selection(i3d_fusion* src, const i3d_register_volume_desc* desc, int64_t capacity, int32_t* keys, float* sdf, int64_t* count) {
    const std::string fn = "i3d_fusion_debug_register_volume_selection";
    if (!src) return I3D_ERR_INVALID_ARGUMENT;
    if (int rc = volume_desc_check(src, fn, desc)) return rc;
    if (capacity < 0 || (capacity > 0 && (!keys || !sdf)) || !count) return fail(src, I3D_ERR_INVALID_ARGUMENT, fn + ": bad arguments");
    VolumePass vp;
    if (int rc = volume_select(src, src, fn, desc, vp)) return rc;
    *count = (int64_t)vp.list.n;
    const size_t m = (size_t)std::min<int64_t>(capacity, (int64_t)vp.list.n);
    if (m == 0) return I3D_OK;
    std::vector<unsigned long long> packed(m);
    F_HIP(src, hipMemcpyAsync(packed.data(), vp.list.keys, m * sizeof(unsigned long long), hipMemcpyDeviceToHost, src->stream));
    F_HIP(src, hipMemcpyAsync(sdf, vp.list.sdf, m * sizeof(float), hipMemcpyDeviceToHost, src->stream));
    F_HIP(src, hipStreamSynchronize(src->stream));
    for (size_t i = 0; i < m; ++i)
        for (int a = 0; a < 3; ++a) keys[3 * i + a] = (int32_t)((packed[i] >> (21 * a)) & 0x1FFFFFull) - FUSION_COORD_OFFSET;
    return I3D_OK;
}

int i3d_fusion_debug_register_volume_sums(i3d_fusion* f, i3d_fusion* src, const i3d_register_volume_desc* desc, const double* pose6, const double* pivot3,
                                          int64_t limit, int32_t row_cap, double* sums29, int64_t* valid, int64_t* selected) {
    const std::string fn = "i3d_fusion_debug_register_volume_sums";
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (!pose6 || !pivot3 || !sums29) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null argument");
    double pose[6];
    for (int k = 0; k < 6; ++k) pose[k] = pose6[k];
    const VolumeDebug dbg{pivot3, limit, row_cap, sums29, valid, selected};
    return register_volume_run(f, src, fn, desc, pose, nullptr, &dbg);
}

}  // extern "C"

// ---- an indexed mesh of the table as it stands ------------------------------------------------------------------------------------------
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

// Section 29.2: the list (flag, scan, gather, sort, slot -> position), the count pass, the two scans, the vertices and the faces, one download.  Three
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
    // per slot: flags | offsets | slot -> position | scan temp | counters
    size_t scan_bytes = 0;
    F_HIP(f, rocprim::exclusive_scan(nullptr, scan_bytes, (int*)nullptr, (int*)nullptr, 0, cap, rocprim::plus<int>(), st));
    const size_t o_flags = 0, o_offs = o_flags + pad(cap * sizeof(int)), o_pos = o_offs + pad(cap * sizeof(int)), o_tmp0 = o_pos + pad(cap * sizeof(int)),
                 o_cnt = o_tmp0 + pad(scan_bytes);
    F_HIP(f, f->mesh_slots.alloc(o_cnt + pad(sizeof(FusionMeshCounters))));
    unsigned char* sb = f->mesh_slots.p;
    int* flags = (int*)(sb + o_flags); int* offs = (int*)(sb + o_offs); int* pos_of_slot = (int*)(sb + o_pos);
    FusionMeshCounters* d_cnt = (FusionMeshCounters*)(sb + o_cnt);
    launch_fusion_mesh_flag(st, t, flags);
    F_HIP(f, hipGetLastError());
    { size_t bytes = scan_bytes; F_HIP(f, rocprim::exclusive_scan(sb + o_tmp0, bytes, flags, offs, 0, cap, rocprim::plus<int>(), st)); }
    F_HIP(f, hipMemsetAsync(pos_of_slot, 0xFF, cap * sizeof(int), st));
    F_HIP(f, hipMemsetAsync(d_cnt, 0, sizeof(FusionMeshCounters), st));
    int last[2] = {0, 0};
    F_HIP(f, hipMemcpyAsync(&last[0], flags + (cap - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipMemcpyAsync(&last[1], offs + (cap - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    const size_t n = (size_t)last[0] + (size_t)last[1];
    i3d_fusion_mesh_stats s; std::memset(&s, 0, sizeof(s));
    s.stored = (int64_t)n;
    MeshData R;
    if (n == 0) { M = std::move(R); out = s; return I3D_OK; }
    // per list entry: keys x2 | slots x2 | kept | face offsets | used [6 n] | vertex ids [6 n] | sort / scan temp
    const size_t nu = n * FUSION_MESH_CODES;
    using UsedIt = rocprim::transform_iterator<const unsigned char*, MeshToLL<unsigned char>, long long>;
    using KeptIt = rocprim::transform_iterator<const int*, MeshToLL<int>, long long>;
    size_t sort_bytes = 0, vscan_bytes = 0, fscan_bytes = 0;
    F_HIP(f, rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, n, 0, 64, st));
    F_HIP(f, rocprim::exclusive_scan(nullptr, vscan_bytes, UsedIt(nullptr, MeshToLL<unsigned char>()), (long long*)nullptr, 0ll, nu, rocprim::plus<long long>(), st));
    F_HIP(f, rocprim::exclusive_scan(nullptr, fscan_bytes, KeptIt(nullptr, MeshToLL<int>()), (long long*)nullptr, 0ll, n, rocprim::plus<long long>(), st));
    const size_t temp = std::max(sort_bytes, std::max(vscan_bytes, fscan_bytes));
    const size_t o_k0 = 0, o_k1 = o_k0 + pad(n * 8), o_s0 = o_k1 + pad(n * 8), o_s1 = o_s0 + pad(n * 4), o_kept = o_s1 + pad(n * 4), o_fat = o_kept + pad(n * 4),
                 o_used = o_fat + pad(n * 8), o_vid = o_used + pad(nu), o_tmp1 = o_vid + pad(nu * 8);
    F_HIP(f, f->mesh_list.alloc(o_tmp1 + pad(temp)));
    unsigned char* lb = f->mesh_list.p;
    unsigned long long* k0 = (unsigned long long*)(lb + o_k0); unsigned long long* k1 = (unsigned long long*)(lb + o_k1);
    unsigned int* s0 = (unsigned int*)(lb + o_s0); unsigned int* s1 = (unsigned int*)(lb + o_s1);
    int* kept = (int*)(lb + o_kept); long long* face_at = (long long*)(lb + o_fat); unsigned char* used = lb + o_used; long long* vertex_id = (long long*)(lb + o_vid);
    launch_fusion_mesh_gather(st, t, flags, offs, (long long)n, k0, s0);
    F_HIP(f, hipGetLastError());
    { size_t bytes = temp; F_HIP(f, rocprim::radix_sort_pairs(lb + o_tmp1, bytes, k0, k1, s0, s1, n, 0, 64, st)); }
    launch_fusion_mesh_positions(st, t, (long long)n, s1, pos_of_slot);
    F_HIP(f, hipGetLastError());
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
    f->render_bricks_ok = false;                                         // the set of slots with weight != 0 may change
    launch_fusion_debug_poke_voxels(st, f->table(), (long long)n, d_keys.p, d_sdf.p, d_w.p, d_rgb.p, d_found.p);
    F_HIP(f, hipGetLastError());
    F_HIP(f, hipMemcpyAsync(found, d_found.p, m, hipMemcpyDeviceToHost, st));
    F_HIP(f, hipStreamSynchronize(st));
    return I3D_OK;
}

}  // extern "C"
