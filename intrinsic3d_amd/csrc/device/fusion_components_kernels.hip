// Connected components of the stored voxels that pass criteria W and S: 6-connectivity over the nodes' slot list in ascending packed key.
//   k_components_init       one lane per entry: parent[j] = the start of j's x-run (bounded look-back) - the packed key has x in its low bits, so the -x neighbour
//                           of entry j, if it is a node, is entry j - 1 with key - 1; no probe, and each lane writes its own word only
//   k_components_link       one lane per entry: the +y and +z neighbours through find_slot and the list's inverse map, each united with the entry by a lock-free
//                           union-find - find both roots, hook the LARGER position under the smaller with a compare-and-swap on a word that still is a root, on
//                           failure go on from the value that came back.  A parent is never above its child, so the root of a tree is its smallest position
//                           whatever the interleaving: the labelling does not depend on the order in which the atomics land (39.1 item 3)
//   k_components_flatten    a launch of its own: parent is read-only there (plain loads), root[j] goes into another array, one writer per word
//   k_components_sizes      size[root] with one integer atomic per wave and distinct root (1-2 on real data: the main surface is one component of millions)
//   k_components_root_keys, _number, _label    one 64-bit key (inverted size, root position) per root for the caller's radix sort, then the numbers
//   k_components_mark       the removal of i3d_fusion_prune_components as one byte per slot for k_prune_rehash (fusion_kernels.hip)
// Visibility in the link launch: the XCDs of gfx950 have private L2s and a CU's L1 is not refreshed by other CUs' stores, so EVERY access to parent there is an
// agent-scope atomic - relaxed loads, the compare-and-swap of a hook, an atomic min for the path halving.  No access needs ordering against another: a stale
// parent is still an ancestor (parents only ever move towards the root), and a hook succeeds only on a word that is a root at that moment.
// Bounded loops: a find walks strictly downwards in position and a failed hook goes on from a smaller position, so n bounds both; a lane that exceeds the bound
// (which a correct parent array cannot cause) sets the error word and ends.  Nothing here waits for another lane.
// No floating point but the selector's comparisons (slot_list.hip); compiled with -ffp-contract=off as the other fusion files.
#include "fusion_components_kernels.hpp"
#include "fusion_hash.hpp"

namespace i3d {
namespace {

constexpr int TPB = 256;              // 4 waves of 64
inline unsigned blocks(long long n) { return (unsigned)((n + TPB - 1) / TPB); }
using namespace fusion_hash;

#define I3D_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
__device__ inline int load_parent(int* parent, int x) { return __hip_atomic_load(&parent[x], I3D_RLX_AGENT); }

// the root of x's tree, halving the path on the way: parent[x] = min(parent[x], grandparent).  -1 if the walk took more than n steps
__device__ inline int find_root(int* parent, int x, int n) {
    int p = load_parent(parent, x);
    for (int steps = 0; p != x; ++steps) {
        if (steps >= n) return -1;
        const int g = load_parent(parent, p);
        if (g != p) __hip_atomic_fetch_min(&parent[x], g, I3D_RLX_AGENT);
        x = p; p = g;
    }
    return x;
}
// 0, or the error code: 1 a find ran out, 2 the hook retries ran out
__device__ inline int unite(int* parent, int a, int b, int n) {
    for (int tries = 0; tries <= n; ++tries) {
        a = find_root(parent, a, n); b = find_root(parent, b, n);
        if (a < 0 || b < 0) return 1;
        if (a == b) return 0;
        if (a < b) { const int s = a; a = b; b = s; }
        int seen = a;
        if (__hip_atomic_compare_exchange_strong(&parent[a], &seen, b, __ATOMIC_RELAXED, I3D_RLX_AGENT)) return 0;
        a = seen;                                     // a has a parent now: go on from it
    }
    return 2;
}

__global__ void __launch_bounds__(TPB) k_components_init(FusionNodeList l, int* __restrict__ parent) {
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= l.n) return;
    int start = (int)j;
    unsigned long long k = l.keys[start];
    for (int i = 0; i < FUSION_COMPONENTS_RUN && start > 0; ++i) {
        const unsigned long long before = l.keys[start - 1];
        if (before + 1ull != k || (k & 0x1FFFFFull) == 0ull) break;      // not the -x neighbour (a carry out of x is no neighbour either)
        --start; k = before;
    }
    parent[j] = start;
}

__global__ void __launch_bounds__(TPB) k_components_link(FusionTable t, FusionNodeList l, int* parent, FusionComponentCounters* cnt) {
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= l.n) return;
    const unsigned long long key = l.keys[j];
    int x, y, z; unpack_key(key, x, y, z);
    const unsigned long long nk[2] = {key + (1ull << 21), key + (1ull << 42)};
    const bool has[2] = {y + 1 < FUSION_COORD_OFFSET, z + 1 < FUSION_COORD_OFFSET};      // the neighbour has a packed key
    // the two home slots together, before the first is looked at: an EMPTY one means the neighbour is not stored
    unsigned long long home[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) home[a] = has[a] ? t.keys[slot_of(nk[a], t.mask)] : FUSION_EMPTY;
    __builtin_amdgcn_sched_barrier(0);
    int err = 0;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if (home[a] == FUSION_EMPTY) continue;
        const long long s = find_slot(t, nk[a]);
        if (s < 0) continue;
        const int pos = l.pos_of_slot[s];
        if (pos < 0 || pos >= l.n) continue;          // stored, but not a node
        const int e = unite(parent, (int)j, pos, l.n);
        if (e > err) err = e;
    }
    if (err) atomicMax(&cnt->error, err);
}

__global__ void __launch_bounds__(TPB) k_components_flatten(int n, const int* __restrict__ parent, int* __restrict__ root, FusionComponentCounters* cnt) {
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    bool is_root = false;
    if (j < n) {
        int x = (int)j, p = parent[x], steps = 0;
        while (p != x && steps < n) { x = p; p = parent[x]; ++steps; }
        if (p != x) atomicMax(&cnt->error, 3);
        root[j] = x;
        is_root = x == (int)j;
    }
    const unsigned long long m = (unsigned long long)__popcll(__ballot(is_root));      // every lane of the wave is here: one atomic per wave
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt->roots, m);
}

__global__ void __launch_bounds__(TPB) k_components_sizes(int n, const int* __restrict__ root, unsigned int* size) {
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int r = j < n ? root[j] : -1;
    unsigned long long todo = __ballot(r >= 0);
    while (todo) {                                    // one turn per distinct root of the wave, 64 at the most
        const int leader = __ffsll((long long)todo) - 1;
        const int lr = __shfl(r, leader);
        const unsigned long long same = __ballot(r == lr);
        if (lane == leader) atomicAdd(&size[lr], (unsigned int)__popcll(same));
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(TPB) k_components_root_keys(int n, long long components, const int* __restrict__ root, const unsigned int* __restrict__ size,
                                                              unsigned long long* __restrict__ sort_keys, FusionComponentCounters* cnt) {
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool is_root = j < n && root[j] == (int)j;
    const unsigned long long mine = __ballot(is_root);
    if (!mine) return;                                // wave-uniform
    const int leader = __ffsll((long long)mine) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(&cnt->cursor, (unsigned long long)__popcll(mine));
    base = __shfl(base, leader);
    if (!is_root) return;
    const unsigned long long at = base + (unsigned long long)__popcll(mine & ((1ull << lane) - 1ull));
    if (at < (unsigned long long)components) sort_keys[at] = ((unsigned long long)(0xFFFFFFFFu - size[j]) << 32) | (unsigned long long)(unsigned int)j;
}

__global__ void __launch_bounds__(TPB) k_components_number(int n, long long components, const unsigned long long* __restrict__ sorted_keys, int* __restrict__ number_of_root,
                                                           long long* __restrict__ sizes) {
    const long long c = (long long)blockIdx.x * TPB + threadIdx.x;
    if (c >= components) return;
    const unsigned long long k = sorted_keys[c];
    const unsigned int at = (unsigned int)(k & 0xFFFFFFFFull);
    if (at < (unsigned int)n) number_of_root[at] = (int)c;
    sizes[c] = (long long)(0xFFFFFFFFu - (unsigned int)(k >> 32));
}

__global__ void __launch_bounds__(TPB) k_components_label(int n, const int* __restrict__ root, const int* __restrict__ number_of_root, int* __restrict__ label) {
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= n) return;
    const int r = root[j];
    label[j] = r >= 0 && r < n ? number_of_root[r] : -1;
}

__global__ void __launch_bounds__(TPB) k_components_mark(FusionNodeList l, unsigned long long mask, const int* __restrict__ label, int first_removed,
                                                         unsigned char* __restrict__ remove) {
    const long long j = (long long)blockIdx.x * TPB + threadIdx.x;
    if (j >= l.n || label[j] < first_removed) return;
    const unsigned int s = l.slots[j];
    if (s <= mask) remove[s] = 1;
}

}  // namespace

void launch_fusion_components_init(hipStream_t st, FusionNodeList l, int* parent) {
    if (l.n > 0) hipLaunchKernelGGL(k_components_init, blocks(l.n), TPB, 0, st, l, parent);
}
void launch_fusion_components_link(hipStream_t st, FusionTable t, FusionNodeList l, int* parent, FusionComponentCounters* cnt) {
    if (l.n > 0) hipLaunchKernelGGL(k_components_link, blocks(l.n), TPB, 0, st, t, l, parent, cnt);
}
void launch_fusion_components_flatten(hipStream_t st, int n, const int* parent, int* root, FusionComponentCounters* cnt) {
    if (n > 0) hipLaunchKernelGGL(k_components_flatten, blocks(n), TPB, 0, st, n, parent, root, cnt);
}
void launch_fusion_components_sizes(hipStream_t st, int n, const int* root, unsigned int* size) {
    if (n > 0) hipLaunchKernelGGL(k_components_sizes, blocks(n), TPB, 0, st, n, root, size);
}
void launch_fusion_components_root_keys(hipStream_t st, int n, long long components, const int* root, const unsigned int* size, unsigned long long* sort_keys,
                                        FusionComponentCounters* cnt) {
    if (n > 0) hipLaunchKernelGGL(k_components_root_keys, blocks(n), TPB, 0, st, n, components, root, size, sort_keys, cnt);
}
void launch_fusion_components_number(hipStream_t st, int n, long long components, const unsigned long long* sorted_keys, int* number_of_root, long long* sizes) {
    if (components > 0) hipLaunchKernelGGL(k_components_number, blocks(components), TPB, 0, st, n, components, sorted_keys, number_of_root, sizes);
}
void launch_fusion_components_label(hipStream_t st, int n, const int* root, const int* number_of_root, int* label) {
    if (n > 0) hipLaunchKernelGGL(k_components_label, blocks(n), TPB, 0, st, n, root, number_of_root, label);
}
void launch_fusion_components_mark(hipStream_t st, FusionNodeList l, unsigned long long mask, const int* label, int first_removed, unsigned char* remove) {
    if (l.n > 0) hipLaunchKernelGGL(k_components_mark, blocks(l.n), TPB, 0, st, l, mask, label, first_removed, remove);
}

}  // namespace i3d
