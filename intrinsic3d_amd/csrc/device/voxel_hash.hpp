// Lookup in the device hash of the resident grid (open addressing, linear probing, filled by k_hash_build in grid_kernels.hip): one definition for every kernel
// that reads it (neighbour table, level transitions, mesh extraction, ray casting).
#pragma once
#include "kernels.hpp"

namespace i3d {

// 21 bits per axis, biased by 2^20
static __device__ __host__ inline unsigned long long pack_key(int x, int y, int z) {
    const unsigned long long B = 1ull << 20;
    return ((unsigned long long)(x + (long long)B) & 0x1fffffull) | (((unsigned long long)(y + (long long)B) & 0x1fffffull) << 21) |
           (((unsigned long long)(z + (long long)B) & 0x1fffffull) << 42);
}
static __device__ inline unsigned int mix64(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (unsigned int)k;
}
// device index of voxel (x, y, z), -1 = not stored
static __device__ inline int hash_find(const HashTable& t, int x, int y, int z) {
    const unsigned long long key = pack_key(x, y, z);
    unsigned int h = mix64(key) & t.mask;
    for (;;) {
        const unsigned long long k = t.keys[h];
        if (k == key) return t.vals[h];
        if (k == ~0ull) return -1;
        h = (h + 1) & t.mask;
    }
}

}  // namespace i3d
