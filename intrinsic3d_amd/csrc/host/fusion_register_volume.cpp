// i3d_fusion_register_volume: one fusion volume aligned to another on the two stored fields (register_volume_kernels.hip).  The samples are
// a slot list of src (section 27.4, the band selector) kept in the handle of the volume registered against; the loop over them is register.cpp's register_loop.
#include "fusion_internal.hpp"
#include "../device/register_volume_kernels.hpp"
#include <algorithm>

using namespace i3d;

namespace {

constexpr long long REGISTER_VOLUME_MAX = 1ll << 27;
constexpr int REGISTER_VOLUME_MAX_ITERATIONS = 200, REGISTER_VOLUME_MAX_STRIDE = 64;

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

// Section 28.1 items 2 and 3 on owner's stream, in owner's slot list: flag, scan, gather, sort by packed key.  One synchronisation, for the count.  owner == src for
// the debug entry that only lists.
int volume_select(i3d_fusion* owner, i3d_fusion* src, const std::string& fn, const i3d_register_volume_desc* d, VolumeList& out) {
    F_HIP(owner, hipSetDevice(owner->device));
    if (owner != src) F_HIP(owner, hipStreamSynchronize(src->stream));          // src is read on owner's stream from here on
    size_t n = 0;
    F_HIP(owner, owner->list.scan(owner->stream, src->table(), SlotBand{d->source_band_voxels * (double)src->voxel_size, d->stride}));
    F_HIP(owner, owner->list.count(n));
    if ((long long)n > REGISTER_VOLUME_MAX)
        return fail(owner, I3D_ERR_CAPACITY, fn + ": " + std::to_string(n) + " voxels selected, more than 2^27: raise stride (now " + std::to_string(d->stride) +
                                                 ") or lower source_band_voxels");
    if (n > 0) F_HIP(owner, owner->list.sort(n));
    out = VolumeList{owner->list.keys(), (const float*)owner->list.payload(), (long long)n, (double)src->voxel_size};
    return I3D_OK;
}

// validation, the selection, then register.cpp's loop over the list: the pivot, the whole budget launched back to back, the figures at the returned pose; three
// synchronisations: the count, the pivot, the result.  dbg: one pass at pose6_io about the given pivot over the first `limit` entries
int register_volume_run(i3d_fusion* f, i3d_fusion* src, const std::string& fn, const i3d_register_volume_desc* d, double* pose6_io, i3d_register_volume_stats* stats,
                        const VolumeDebug* dbg) {
    if (!f) return I3D_ERR_INVALID_ARGUMENT;
    if (int rc = two_volumes_check(f, src, fn, pose6_io, "registered to")) return rc;
    if (int rc = volume_desc_check(f, fn, d)) return rc;
    if (!pose6_io) return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": null pose");
    if (dbg && (dbg->limit < 0 || dbg->row_cap < 0 || dbg->row_cap > REGISTER_MAX_ROWS))
        return fail(f, I3D_ERR_INVALID_ARGUMENT, fn + ": limit must be >= 0 and row_cap 0..8192 (0: all / the default)");

    VolumeList list;
    if (int rc = volume_select(f, src, fn, d, list)) return rc;
    hipStream_t st = f->stream;
    i3d_register_volume_stats out; std::memset(&out, 0, sizeof(out));
    out.status = 2; out.selected = (int64_t)list.n;
    if (dbg) {
        if (dbg->sums29) std::memset(dbg->sums29, 0, TRACK_SUMS * sizeof(double));
        if (dbg->valid) *dbg->valid = 0;
        if (dbg->selected) *dbg->selected = out.selected;
    }
    const long long n = dbg && dbg->limit > 0 && dbg->limit < list.n ? (long long)dbg->limit : list.n;
    if (n == 0) { if (stats) *stats = out; return I3D_OK; }      // an empty src, or nothing selected: status 2 without a sums launch

    // the scratch: slab | state
    const int row_cap = dbg && dbg->row_cap > 0 ? dbg->row_cap : REGISTER_MAX_ROWS;
    const int P = register_per_lane(n, row_cap), rows = register_rows(n, P);
    const size_t o_state = ((size_t)rows * TRACK_COLS * sizeof(double) + 255) & ~(size_t)255;
    F_HIP(f, f->register_volume_scratch.alloc(o_state + sizeof(TrackState)));
    double* slab = (double*)f->register_volume_scratch.p;
    TrackState* state = (TrackState*)(f->register_volume_scratch.p + o_state);
    const FusionRenderGrid g = field_grid(f);

    RegisterLoop lp;
    lp.slab = slab; lp.state = state; lp.n = n; lp.per_lane = P;
    lp.mean = [&](const double* R0, const double* t0) { launch_register_volume_mean(st, list, P, R0, t0, g.vs, slab); };      // x_f = R x_src + t
    lp.pass = [&](const RegisterParams& prm, int check_done) { launch_register_volume(st, g, prm, list, state, check_done, slab); };
    lp.iterations = d->iterations; lp.stop_rotation = d->stop_rotation; lp.stop_translation = d->stop_translation; lp.max_distance = d->max_distance;
    if (dbg) { lp.debug_pivot3 = dbg->pivot3; lp.debug_sums29 = dbg->sums29; lp.debug_valid = dbg->valid; }
    i3d_register_stats r; std::memset(&r, 0, sizeof(r));
    if (int rc = register_loop(FusionModel(f, fn), lp, pose6_io, r)) return rc;
    if (dbg) return I3D_OK;
    out.valid = r.valid; out.inliers = r.inliers; out.rms_initial = r.rms_initial; out.rms_final = r.rms_final; out.iterations = r.iterations;
    out.min_pivot_ratio = r.min_pivot_ratio; out.status = r.status;
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
    VolumeList list;
    if (int rc = volume_select(src, src, fn, desc, list)) return rc;
    *count = (int64_t)list.n;
    const size_t m = (size_t)std::min<int64_t>(capacity, (int64_t)list.n);
    if (m == 0) return I3D_OK;
    std::vector<unsigned long long> packed(m);
    F_HIP(src, hipMemcpyAsync(packed.data(), list.keys, m * sizeof(unsigned long long), hipMemcpyDeviceToHost, src->stream));
    F_HIP(src, hipMemcpyAsync(sdf, list.sdf, m * sizeof(float), hipMemcpyDeviceToHost, src->stream));
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
