// Connected components of the stored voxels of a fusion volume: a lock-free union-find over the nodes' slot list (slot_list.hpp, SlotNode)
// in ascending packed key.  Launch wrappers of fusion_components_kernels.hip; the host around them is host/fusion_components.cpp.
#pragma once
#include "fusion_kernels.hpp"

namespace i3d {

// the nodes as the kernels read them: keys and slots in ascending packed key (a slot list whose payload is the slot), and the list's inverse map [capacity], -1
// where the slot holds no node
struct FusionNodeList {
    const unsigned long long* keys; const unsigned int* slots; const int* pos_of_slot; int n;
};
// what the launches count: zeroed by the caller before init
struct FusionComponentCounters {
    unsigned long long roots;                                // entries that are their own root = components (flatten)
    unsigned long long cursor;                               // where the next wave puts its roots' sort keys (root_keys)
    int error;                                               // != 0: a bounded loop ran out (link: 1 find, 2 hook; flatten: 3); the labelling is not to be used
    int pad;
};

// parent[j] = the start of j's x-run, at most FUSION_COMPONENTS_RUN entries back, or j: entry j - 1 is the -x neighbour iff its key is keys[j] - 1
constexpr int FUSION_COMPONENTS_RUN = 16;
void launch_fusion_components_init(hipStream_t st, FusionNodeList l, int* parent);
// one lane per entry: the +y and +z neighbours by lookup, each united with the entry; afterwards the root of every tree is its smallest position
void launch_fusion_components_link(hipStream_t st, FusionTable t, FusionNodeList l, int* parent, FusionComponentCounters* cnt);
// root[j] = the root of j's tree (parent is only read); cnt->roots += the entries that are their own root
void launch_fusion_components_flatten(hipStream_t st, int n, const int* parent, int* root, FusionComponentCounters* cnt);
// size[r] += the entries with root r (the caller zeroes size [n]): one atomic per wave and distinct root
void launch_fusion_components_sizes(hipStream_t st, int n, const int* root, unsigned int* size);
// one 64-bit sort key per root into sort_keys [components = cnt->roots after flatten], in no particular order: (~size) << 32 | root position; ascending = descending size, ties by ascending smallest packed key
void launch_fusion_components_root_keys(hipStream_t st, int n, long long components, const int* root, const unsigned int* size, unsigned long long* sort_keys,
                                        FusionComponentCounters* cnt);
// one lane per component of the sorted keys: number_of_root[root position] = c, sizes[c] = its size
void launch_fusion_components_number(hipStream_t st, int n, long long components, const unsigned long long* sorted_keys, int* number_of_root, long long* sizes);
// label[j] = number_of_root[root[j]]
void launch_fusion_components_label(hipStream_t st, int n, const int* root, const int* number_of_root, int* label);
// remove[slots[j]] = 1 where label[j] >= first_removed (the caller zeroes remove [mask + 1]); one writer per slot
void launch_fusion_components_mark(hipStream_t st, FusionNodeList l, unsigned long long mask, const int* label, int first_removed, unsigned char* remove);

}  // namespace i3d
