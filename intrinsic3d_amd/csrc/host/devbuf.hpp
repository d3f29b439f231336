// Device and pinned host memory owned by a handle, grown only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace i3d {

template <class T>
struct DevBuf {
    T* p = nullptr; size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t count) {          // grow-only
        if (count <= n && p) return hipSuccess;
        release();
        if (count == 0) return hipSuccess;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
};

// pinned host memory, grown only: what a driver stages there goes to and from the device by copies that are enqueued, not staged
struct PinnedBuf {
    unsigned char* p = nullptr; size_t n = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete; PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { release(); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
    hipError_t alloc(size_t bytes) {
        if (bytes <= n) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc((void**)&p, bytes);
        if (e == hipSuccess) n = bytes;
        return e;
    }
};

}  // namespace i3d
