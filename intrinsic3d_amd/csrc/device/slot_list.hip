// The selected slots of the fusion table as a list (slot_list.hpp):
//   k_slot_flag<Sel>    one lane per slot: 1 where the selector takes the slot
//   k_slot_gather<Sel>  one lane per slot: the selector's (key, payload) of a flagged slot at its scanned offset, where that lies inside the buffers
//   k_slot_positions    one lane per list entry: slot -> list position, the inverse map of a list whose payload is the slot
// Compiled with -ffp-contract=off as the files the selectors came from; the band test is a comparison of a converted float, nothing here multiplies and adds.
#include "slot_list.hpp"

namespace i3d {
namespace {

constexpr int SLOT_BLOCK = 256;       // 4 waves of 64
inline unsigned slot_blocks(unsigned long long n) { return (unsigned)((n + SLOT_BLOCK - 1) / SLOT_BLOCK); }

template <class Sel>
__global__ void __launch_bounds__(SLOT_BLOCK) k_slot_flag(FusionTable t, Sel sel, int* __restrict__ flags) {
    const unsigned long long i = (unsigned long long)blockIdx.x * SLOT_BLOCK + threadIdx.x;
    if (i > t.mask) return;
    flags[i] = sel.selected(t, i) ? 1 : 0;
}

template <class Sel>
__global__ void __launch_bounds__(SLOT_BLOCK) k_slot_gather(FusionTable t, Sel sel, const int* __restrict__ flags, const int* __restrict__ offs, long long n,
                                                            unsigned long long* __restrict__ keys, unsigned int* __restrict__ payload) {
    const unsigned long long i = (unsigned long long)blockIdx.x * SLOT_BLOCK + threadIdx.x;
    if (i > t.mask || !flags[i]) return;
    const long long at = offs[i];
    if (at < 0 || at >= n) return;                   // n = the scanned count: the buffers' size
    keys[at] = sel.key(t, i); payload[at] = sel.payload(t, i);
}

__global__ void __launch_bounds__(SLOT_BLOCK) k_slot_positions(long long n, unsigned long long mask, const unsigned int* __restrict__ slot_sorted,
                                                               int* __restrict__ pos_of_slot) {
    const long long i = (long long)blockIdx.x * SLOT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned int s = slot_sorted[i];
    if (s <= mask) pos_of_slot[s] = (int)i;
}

}  // namespace

template <class Sel> void launch_slot_flag(hipStream_t st, FusionTable t, Sel sel, int* flags) {
    k_slot_flag<Sel><<<slot_blocks(t.mask + 1), SLOT_BLOCK, 0, st>>>(t, sel, flags);
}
template <class Sel> void launch_slot_gather(hipStream_t st, FusionTable t, Sel sel, const int* flags, const int* offsets, long long n, unsigned long long* keys,
                                             unsigned int* payload) {
    k_slot_gather<Sel><<<slot_blocks(t.mask + 1), SLOT_BLOCK, 0, st>>>(t, sel, flags, offsets, n, keys, payload);
}
void launch_slot_positions(hipStream_t st, FusionTable t, long long n, const unsigned int* slot_sorted, int* pos_of_slot) {
    if (n > 0) k_slot_positions<<<slot_blocks(n), SLOT_BLOCK, 0, st>>>(n, t.mask, slot_sorted, pos_of_slot);
}

#define I3D_SLOT_SELECTOR(Sel) \
    template void launch_slot_flag<Sel>(hipStream_t, FusionTable, Sel, int*); \
    template void launch_slot_gather<Sel>(hipStream_t, FusionTable, Sel, const int*, const int*, long long, unsigned long long*, unsigned int*);
I3D_SLOT_SELECTOR(SlotStored) I3D_SLOT_SELECTOR(SlotInserted) I3D_SLOT_SELECTOR(SlotWeighted) I3D_SLOT_SELECTOR(SlotBand) I3D_SLOT_SELECTOR(SlotNode)
#undef I3D_SLOT_SELECTOR

}  // namespace i3d
