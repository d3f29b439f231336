"""numpy statement of i3d_fusion_insert_records / i3d_fusion_snapshot, no device involved.

The record order of a volume is the iteration order of the reference's unordered_map after it received the keys in their insertion sequence.  Mode 2 of
i3d_debug_map_order is a real std::unordered_map on the host: it shares no code with the device replay that finish and snapshot run."""
import numpy as np

from intrinsic3d_amd import binding as B


def pack(keys):
    k = np.asarray(keys, np.int64).reshape(-1, 3) + (1 << 20)
    return k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)


def order(seq_keys, mode=2):
    """the keys in the iteration order of an unordered_map that received them in the order given"""
    k = np.ascontiguousarray(seq_keys, np.int32).reshape(-1, 3)
    return k[B.debug_map_order(k, mode=mode)] if len(k) else k


def loaded(records):
    """the volume after insert_records into an empty one: a dict by packed key of (sdf, weight, colour, first_frame = 0), weight-0 records included"""
    keys = np.asarray(records["keys"], np.int32).reshape(-1, 3)
    vol = {}
    for p, s, w, c in zip(pack(keys).tolist(), records["sdf"], records["weight"], np.asarray(records["color"]).reshape(-1, 3)):
        assert p not in vol, "a key appears twice"
        vol[p] = (np.float32(s), np.float32(w), tuple(int(x) for x in c), 0)
    return vol


def snapshot_records(volume, seq_keys):
    """the records of snapshot / finish(0): the voxels of weight > 0 in order(seq_keys).  volume: dict by packed key of (sdf, weight, colour, ..); seq_keys: the
    insertion sequence of ALL stored voxels"""
    k = order(seq_keys)
    rec = [volume[p] for p in pack(k).tolist()]
    keep = np.array([r[1] > 0 for r in rec], bool) if rec else np.zeros(0, bool)
    return dict(keys=np.ascontiguousarray(k[keep]),
                sdf=np.array([r[0] for r, on in zip(rec, keep) if on], np.float32),
                weight=np.array([r[1] for r, on in zip(rec, keep) if on], np.float32),
                color=np.array([r[2] for r, on in zip(rec, keep) if on], np.uint8).reshape(-1, 3))


def volume_of(keys, sdf, weight, color, first_frame):
    """a dict by packed key from the arrays of Fusion.debug_voxels at the found keys"""
    return {p: (np.float32(s), np.float32(w), tuple(int(x) for x in c), int(f))
            for p, s, w, c, f in zip(pack(keys).tolist(), sdf, weight, np.asarray(color).reshape(-1, 3), first_frame)}
