// "The selected slots of the fusion table as a sorted list" (DESIGN.md section 27.4): one lane per slot flags the selected ones, the caller's exclusive scan gives
// each its place, one lane per slot gathers a 64-bit sort key and a 32-bit payload there, the caller's radix sort over 64 bits orders the pairs.  What is selected,
// and what key and payload an entry carries, is a selector passed by value.  Launch wrappers of slot_list.hip; the buffers and the scan and sort around the kernels
// are host/fusion_internal.hpp's SlotList.
#pragma once
#include "fusion_hash.hpp"

namespace i3d {

// every stored voxel, in the order of first insertion (i3d_fusion_finish)
struct SlotStored {
    __device__ bool selected(const FusionTable& t, unsigned long long i) const { return t.keys[i] != FUSION_EMPTY; }
    __device__ unsigned long long key(const FusionTable& t, unsigned long long i) const { return t.rank[i]; }
    __device__ unsigned int payload(const FusionTable&, unsigned long long i) const { return (unsigned int)i; }
};
// the voxels the operation with this ordinal inserted: bits 41.. of their rank carry it and no other voxel's do; in ascending packed key (i3d_fusion_merge, 27.2)
struct SlotInserted {
    unsigned long long ordinal;
    __device__ bool selected(const FusionTable& t, unsigned long long i) const { return t.keys[i] != FUSION_EMPTY && (t.rank[i] >> 41) == ordinal; }
    __device__ unsigned long long key(const FusionTable& t, unsigned long long i) const { return t.keys[i]; }
    __device__ unsigned int payload(const FusionTable&, unsigned long long i) const { return (unsigned int)i; }
};
// the stored voxels with weight != 0, in ascending packed key (i3d_fusion_extract_mesh, 29.2)
struct SlotWeighted {
    __device__ bool selected(const FusionTable& t, unsigned long long i) const { return t.keys[i] != FUSION_EMPTY && t.weight[i] != 0.0f; }
    __device__ unsigned long long key(const FusionTable& t, unsigned long long i) const { return t.keys[i]; }
    __device__ unsigned int payload(const FusionTable&, unsigned long long i) const { return (unsigned int)i; }
};
// the nodes of i3d_fusion_components (39.1 item 1): the stored voxels that pass criteria W and S of i3d_fusion_prune (prune_fails_ws, the one definition), in
// ascending packed key
struct SlotNode {
    FusionPrune p;                                // min_weight, max_abs_sdf and their two switches; the box is not looked at
    __device__ bool selected(const FusionTable& t, unsigned long long i) const { return t.keys[i] != FUSION_EMPTY && prune_fails_ws(p, t.weight[i], t.sdf[i]) == 0u; }
    __device__ unsigned long long key(const FusionTable& t, unsigned long long i) const { return t.keys[i]; }
    __device__ unsigned int payload(const FusionTable&, unsigned long long i) const { return (unsigned int)i; }
};
// the samples of i3d_fusion_register_volume (28.1 item 2), in ascending packed key; the payload is the bits of the stored sdf
struct SlotBand {
    double band;                                  // source_band_voxels * (double)src voxel size: a slot is selected when fabs((double)sdf) <= band
    int stride;                                   // and every coordinate is a multiple of stride (floor modulus)
    __device__ static bool on_stride(int k, int stride) {          // floor modulus: -4 is on stride 2 and on stride 4, -3 on neither
        int m = k % stride;
        if (m < 0) m += stride;
        return m == 0;
    }
    __device__ bool selected(const FusionTable& t, unsigned long long i) const {
        const unsigned long long key = t.keys[i];
        if (key == FUSION_EMPTY || t.weight[i] == 0.0f) return false;
        if (!(fabs((double)t.sdf[i]) <= band)) return false;             // also a NaN
        int kx, ky, kz; fusion_hash::unpack_key(key, kx, ky, kz);
        return on_stride(kx, stride) && on_stride(ky, stride) && on_stride(kz, stride);
    }
    __device__ unsigned long long key(const FusionTable& t, unsigned long long i) const { return t.keys[i]; }
    __device__ unsigned int payload(const FusionTable& t, unsigned long long i) const { return __float_as_uint(t.sdf[i]); }
};

// flags: [capacity], 1 where the slot is selected.  Instantiated for the five selectors above
template <class Sel> void launch_slot_flag(hipStream_t st, FusionTable t, Sel sel, int* flags);
// keys / payload: [n]; an entry is written at its scanned offset only where 0 <= offset < n, n being the buffers' size
template <class Sel> void launch_slot_gather(hipStream_t st, FusionTable t, Sel sel, const int* flags, const int* offsets, long long n, unsigned long long* keys,
                                             unsigned int* payload);
// the list's inverse map, for a list whose payload is the slot: pos_of_slot[slot_sorted[j]] = j; pos_of_slot is [capacity], preset to -1 by the caller
void launch_slot_positions(hipStream_t st, FusionTable t, long long n, const unsigned int* slot_sorted, int* pos_of_slot);

}  // namespace i3d
