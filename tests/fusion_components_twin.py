"""numpy statement of i3d_fusion_components / i3d_fusion_prune_components, no device involved.

Test infrastructure: the kernels of fusion_components_kernels.hip are compared against this bit for bit.  The device runs a lock-free union-find with hooks by
compare-and-swap; this file does something else on purpose: the edges come from a binary search in the sorted packed keys, and the labels from rounds of "every
edge pulls both ends and both ends' labels down to the smaller label" followed by pointer jumping until nothing moves.  A label never exceeds its index and never
leaves its component, so the fixed point is the smallest index of the component - which, the nodes being sorted by packed key, is its smallest packed key.

A volume is the dict of arrays fusion_cases.snapshot returns (keys [n, 3], sdf, weight, ...) in any order."""
import numpy as np

import fusion_prune_twin as PT

F = np.float32
COUNTS = ("stored", "removed", "nodes", "components", "components_removed")


def nodes(sdf, weight, min_weight=0.0, max_abs_sdf=0.0):
    """item 1: the mask of the voxels that pass criteria W and S of i3d_fusion_prune - its verdict with the box off"""
    n = len(np.asarray(sdf).reshape(-1))
    return PT.verdict(np.zeros((n, 3), np.int64), sdf, weight, 1.0, min_weight=min_weight, max_abs_sdf=max_abs_sdf) == 0


def _labels(pk):
    """pk: distinct packed keys, ascending.  Per node the smallest index of its 6-connected component."""
    n = len(pk)
    ea, eb = [], []
    for a in range(3):
        coord = (pk >> (21 * a)) & ((1 << 21) - 1)
        want = pk + (1 << (21 * a))
        at = np.minimum(np.searchsorted(pk, want), n - 1)
        hit = (pk[at] == want) & (coord + 1 < (1 << 21))
        ea.append(np.flatnonzero(hit)); eb.append(at[hit])
    ea = np.concatenate(ea); eb = np.concatenate(eb)
    L = np.arange(n, dtype=np.int64)
    while True:
        la, lb = L[ea], L[eb]
        m = np.minimum(la, lb)
        N = L.copy()
        for target in (ea, eb, la, lb):
            np.minimum.at(N, target, m)
        while True:
            J = N[N]
            if np.array_equal(J, N):
                break
            N = J
        if np.array_equal(N, L):
            return L
        L = N


def components(volume, voxel_size=None, min_weight=0.0, max_abs_sdf=0.0):
    """items 1-3: dict(nodes, components, largest, keys [nodes, 3] int32 in ascending packed key, label [nodes] int32, sizes [components] int64)"""
    keys = np.asarray(volume["keys"], np.int64).reshape(-1, 3)
    on = nodes(volume["sdf"], volume["weight"], min_weight, max_abs_sdf) if len(keys) else np.zeros(0, bool)
    pk = np.sort(PT.pack(keys[on]))
    n = len(pk)
    if n == 0:
        return dict(nodes=0, components=0, largest=0, keys=np.zeros((0, 3), np.int32), label=np.zeros(0, np.int32), sizes=np.zeros(0, np.int64))
    assert len(np.unique(pk)) == n, "the keys of a volume are distinct"
    L = _labels(pk)
    roots, size = np.unique(L, return_counts=True)                # roots ascending = ascending smallest packed key
    order = np.lexsort((roots, -size))                            # descending size, ties by ascending smallest packed key
    number = np.empty(n, np.int64); number[roots[order]] = np.arange(len(roots))
    sizes = size[order].astype(np.int64)
    return dict(nodes=n, components=len(roots), largest=int(sizes[0]), keys=PT.unpack(pk).astype(np.int32), label=number[L].astype(np.int32), sizes=sizes)


def removed_components(sizes, min_voxels=0, keep_largest=0):
    """item 5: the mask over the component numbers"""
    c = np.arange(len(sizes))
    return ((min_voxels > 0) & (np.asarray(sizes) < min_voxels)) | ((keep_largest > 0) & (c >= keep_largest))


def prune_components(volume, seq_keys, voxel_size=None, min_weight=0.0, max_abs_sdf=0.0, min_voxels=0, keep_largest=0):
    """(surviving volume, surviving insertion sequence, counts5): fusion_prune_twin.prune with the component verdict as its mask - the mask goes in as the weight
    of a stand-in volume (0 = leaves) under prune's default criterion, and the survivors' indices come back with it"""
    keys = np.asarray(volume["keys"], np.int64).reshape(-1, 3)
    c = components(volume, voxel_size, min_weight, max_abs_sdf)
    gone_c = removed_components(c["sizes"], min_voxels, keep_largest)
    gone_keys = PT.pack(c["keys"][gone_c[c["label"]]]) if c["nodes"] else np.zeros(0, np.int64)
    leaves = np.isin(PT.pack(keys), gone_keys)
    stand_in = dict(keys=keys, sdf=np.zeros(len(keys), F), weight=np.where(leaves, F(0), F(1)), index=np.arange(len(keys)))
    kept, seq, counts = PT.prune(stand_in, seq_keys, voxel_size=1.0)
    assert counts[1] == int(leaves.sum()) == int(c["sizes"][gone_c].sum())
    out = {k: np.asarray(a)[kept["index"]] for k, a in volume.items()}
    return out, seq, [len(keys), int(leaves.sum()), c["nodes"], c["components"], int(gone_c.sum())]
