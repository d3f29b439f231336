// The open-addressing table of the fusion volume (FusionTable, 64-bit packed keys, linear probing): one definition of the key packing, the home slot and the
// lookup for every kernel that reads or writes it (allocation, integration and correctSDF in fusion_kernels.hip; the ray cast of the volume in render_kernels.hip).
#pragma once
#include "fusion_kernels.hpp"

namespace i3d {
namespace fusion_hash {

__device__ inline unsigned long long pack_key(int x, int y, int z) {
    return (unsigned long long)(unsigned)(x + FUSION_COORD_OFFSET) | ((unsigned long long)(unsigned)(y + FUSION_COORD_OFFSET) << 21) |
           ((unsigned long long)(unsigned)(z + FUSION_COORD_OFFSET) << 42);
}
__device__ inline void unpack_key(unsigned long long k, int& x, int& y, int& z) {
    x = (int)(k & 0x1FFFFFull) - FUSION_COORD_OFFSET; y = (int)((k >> 21) & 0x1FFFFFull) - FUSION_COORD_OFFSET; z = (int)((k >> 42) & 0x1FFFFFull) - FUSION_COORD_OFFSET;
}
// Home slot: a multiplicative hash of the packed key.  (A brick-local layout — 512 contiguous slots per 8x8x8 brick — was measured and
// rejected: the surface shell fills long runs of such a group, colliding bricks then probe linearly through hundreds of occupied slots,
// and both allocation and correctSDF became ~40x slower.)
__device__ inline unsigned long long slot_of(unsigned long long key, unsigned long long mask) { return ((key * 0x9E3779B97F4A7C15ull) >> 17) & mask; }
// slot of `key`, -1 = not stored
__device__ inline long long find_slot(const FusionTable& t, unsigned long long key) {
    unsigned long long s = slot_of(key, t.mask);
    for (unsigned long long probes = 0; probes <= t.mask; ++probes) {      // bounded: a completely full table has no empty slot to stop at
        const unsigned long long k = t.keys[s];
        if (k == key) return (long long)s;
        if (k == FUSION_EMPTY) return -1;
        s = (s + 1) & t.mask;
    }
    return -1;
}

}  // namespace fusion_hash
}  // namespace i3d
