// What every model shares behind the model view (model.hpp): the device made current, the intensity volume, the descriptor checks more
// than one driver makes, and the cached brick bitmap.
#include "model.hpp"
#include <climits>

namespace i3d {

int Model::make_current() const {
    MODEL_HIP(*this, hipSetDevice(device));
    return I3D_OK;
}

int Model::fill_intensity(const double*& vol) const {
    MODEL_HIP(*this, buf.intensity.alloc(intensity_entries()));
    launch_intensity(buf.intensity.p);
    vol = buf.intensity.p;
    return I3D_OK;
}

int Model::check_focal(const double* intr) const {
    return intr[0] > 0.0 && intr[1] > 0.0 ? I3D_OK : fail(I3D_ERR_INVALID_ARGUMENT, fn + ": focal lengths must be > 0");
}

int Model::check_pose(const double* pose6) const {
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(pose6[k])) return fail(I3D_ERR_INVALID_ARGUMENT, fn + ": the pose is not finite");
    return I3D_OK;
}

int Model::check_weights(double wg, double wp) const {
    if (!std::isfinite(wg) || !std::isfinite(wp) || wg < 0.0 || wp < 0.0) return fail(I3D_ERR_INVALID_ARGUMENT, fn + ": the weights must be finite and >= 0");
    if (wg == 0.0 && wp == 0.0) return fail(I3D_ERR_INVALID_ARGUMENT, fn + ": both weights are 0");
    return I3D_OK;
}

int ensure_bricks(const Model& m) {
    ModelBuffers::Bricks& k = m.buf.bricks;
    if (k.ok) return I3D_OK;
    hipStream_t st = m.stream;
    const int init[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
    int b[6];
    MODEL_HIP(m, k.bounds.alloc(6));
    MODEL_HIP(m, hipMemcpyAsync(k.bounds.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    m.brick_bounds(k.bounds.p);
    MODEL_HIP(m, hipGetLastError());
    MODEL_HIP(m, hipMemcpyAsync(b, k.bounds.p, sizeof(b), hipMemcpyDeviceToHost, st));
    MODEL_HIP(m, hipStreamSynchronize(st));
    for (int a = 0; a < 3; ++a) { k.lo[a] = 0; k.dim[a] = 0; }
    if (b[0] <= b[3]) {                          // else nothing has a weight: the box is empty and every ray misses
        long long bits = 1;
        for (int a = 0; a < 3; ++a) { k.lo[a] = b[a]; k.dim[a] = b[3 + a] - b[a] + 1; bits *= k.dim[a]; }
        if (bits > (1ll << 31)) {
            for (int a = 0; a < 3; ++a) k.dim[a] = 0;
            return m.fail(I3D_ERR_CAPACITY, std::string(m.bitmap_owner) + ": the brick bitmap of the " + m.noun + "'s bounding box would exceed 2^31 bits (" +
                                                std::to_string(bits) + ")");
        }
        const size_t words = (size_t)((bits + 31) / 32);
        MODEL_HIP(m, k.bits.alloc(words));
        MODEL_HIP(m, hipMemsetAsync(k.bits.p, 0, words * sizeof(unsigned), st));
        m.brick_fill(k.bits.p, k.lo, k.dim);
        MODEL_HIP(m, hipGetLastError());
    }
    k.ok = true;
    return I3D_OK;
}

}  // namespace i3d
