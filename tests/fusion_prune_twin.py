"""numpy statement of i3d_fusion_prune, no device involved.

Test infrastructure: prune_verdict / k_prune_count / k_prune_rehash (fusion_kernels.hip) are compared against this bit for bit.  Every comparison is one IEEE
float32 operation as item 1 writes it.  A volume is either the dict of arrays fusion_cases.snapshot returns (keys [n, 3], sdf, weight, color, first_frame) or the
dict by packed key fusion_load_twin.volume_of returns; prune() gives back the shape it was given."""
import numpy as np

F = np.float32
W, S, B = 1, 2, 4                                    # the bits of a verdict


def pack(keys):
    k = np.asarray(keys, np.int64).reshape(-1, 3) + (1 << 20)
    return k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)


def unpack(p):
    p = np.asarray(p, np.int64); m = (1 << 21) - 1
    return np.stack([p & m, (p >> 21) & m, (p >> 42) & m], -1) - (1 << 20)


def mode_of(box, box_mode):
    """the binding's rule: a given box with no mode means mode 1"""
    return (0 if box is None else 1) if box_mode is None else int(box_mode)


def outside(keys, voxel_size, box):
    """the allocation's clip test: the float32 world coordinate of the voxel against the box, faces inclusive"""
    b = np.asarray(box, F).reshape(6); w = np.asarray(keys).reshape(-1, 3).astype(F) * F(voxel_size)
    return (w[:, 0] < b[0]) | (w[:, 0] > b[1]) | (w[:, 1] < b[2]) | (w[:, 1] > b[3]) | (w[:, 2] < b[4]) | (w[:, 2] > b[5])


def verdict(keys, sdf, weight, voxel_size, min_weight=0.0, max_abs_sdf=0.0, box=None, box_mode=None):
    """item 1: per voxel the mask of the enabled criteria it fails (W = 1, S = 2, B = 4); removed iff != 0"""
    n = len(np.asarray(sdf).reshape(-1))
    v = np.zeros(n, np.uint8)
    s = np.asarray(sdf, F).reshape(n); w = np.asarray(weight, F).reshape(n)
    if F(min_weight) >= F(0):
        v |= np.where(~(w > F(min_weight)), W, 0).astype(np.uint8)
    if F(max_abs_sdf) > F(0):
        v |= np.where(np.abs(s) > F(max_abs_sdf), S, 0).astype(np.uint8)
    mode = mode_of(box, box_mode)
    assert mode in (0, 1, 2)
    if mode != 0:
        out = outside(keys, voxel_size, box)
        v |= np.where(out if mode == 1 else ~out, B, 0).astype(np.uint8)
    return v


def counts_of(v):
    """item 2: stored before, removed, failed W, failed S, failed B; a voxel failing several criteria counts in each"""
    return [int(len(v)), int((v != 0).sum()), int((v & W != 0).sum()), int((v & S != 0).sum()), int((v & B != 0).sum())]


def capacity_after(capacity, kept, removed, shrink):
    """item 6: unchanged without shrink or when nothing goes; else i3d_fusion_create's rule for initial_capacity = kept, never above the current capacity"""
    if not shrink or removed == 0:
        return int(capacity)
    cap = 1 << 12
    while cap < 2 * kept:
        cap <<= 1
    return int(min(cap, capacity))


def prune(volume, seq_keys, voxel_size=None, **params):
    """(surviving volume, surviving insertion sequence, counts5): survivors keep everything they hold (items 4 and 7), the sequence is the old one less the
    removed keys (item 8)"""
    seq = np.asarray(seq_keys, np.int32).reshape(-1, 3)
    by_key = "keys" not in volume
    if by_key:
        pk = np.array(list(volume.keys()), np.int64); keys = unpack(pk) if len(pk) else np.zeros((0, 3), np.int64)
        sdf = np.array([volume[p][0] for p in pk.tolist()], F); weight = np.array([volume[p][1] for p in pk.tolist()], F)
    else:
        keys = np.asarray(volume["keys"], np.int64).reshape(-1, 3); pk = pack(keys); sdf, weight = volume["sdf"], volume["weight"]
    v = verdict(keys, sdf, weight, voxel_size, **params)
    keep = v == 0
    gone = pk[~keep]
    if by_key:
        out = {p: volume[p] for p, k in zip(pk.tolist(), keep) if k}
    else:
        out = {k: np.asarray(a)[keep] for k, a in volume.items()}
    assert len(seq) == len(pk) and np.array_equal(np.sort(pack(seq)), np.sort(pk)), "the sequence must name exactly the stored voxels"
    return out, np.ascontiguousarray(seq[~np.isin(pack(seq), gone)]), counts_of(v)
