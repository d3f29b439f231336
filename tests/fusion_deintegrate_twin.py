"""The update rules of i3d_fusion_deintegrate / i3d_fusion_reintegrate in numpy float32: every operation is one IEEE fp32
operation in the kernels' order, so the statement is exact by construction.  A state is dict(sdf f32 [n], weight f32 [n], color u8 [n, 3]); the samples of a frame are
dict(on bool [n], sample f32 [n], wu f32 [n], has_color bool [n], rgb u8 [n, 3]) (Fusion.debug_frame_samples).  Also the bookkeeping the tests share: packed keys,
lookups in an export, the first frame of every voxel from per-frame exports, and the error bounds of section 23.3."""
import numpy as np

F = np.float32
EPS = 2.0 ** -23


def integrate(state, smp, sel=None):
    """k_integrate's update where smp["on"] (and sel): the running weighted mean, colour truncated"""
    on = smp["on"] if sel is None else smp["on"] & sel
    w_old = state["weight"]; wu = np.where(on, smp["wu"], F(1)).astype(F); w_new = w_old + wu
    sdf = (state["sdf"] * w_old + smp["sample"] * wu) / w_new
    col = ((state["color"].astype(F) * w_old[:, None] + smp["rgb"].astype(F) * wu[:, None]) / w_new[:, None]).astype(np.uint8)
    oc = on & smp["has_color"]
    return dict(sdf=np.where(on, sdf, state["sdf"]), weight=np.where(on, w_new, w_old), color=np.where(oc[:, None], col, state["color"]))


def deintegrate(state, smp, first_frame, ordinal, first_frame_rule=True):
    """k_deintegrate's update where the gates pass and the voxel's first frame is not after `ordinal`; below a weight of 0.5 the voxel is Voxel() again"""
    on = smp["on"] & ((first_frame <= ordinal) if first_frame_rule else True)
    w_old = state["weight"]; wu = np.where(on, smp["wu"], F(0)).astype(F); w_new = w_old - wu
    reset = on & (w_new < F(0.5)); keep = on & ~reset
    den = np.where(keep, w_new, F(1)).astype(F)
    sdf = (state["sdf"] * w_old - smp["sample"] * wu) / den
    col = np.minimum(np.maximum((state["color"].astype(F) * w_old[:, None] - smp["rgb"].astype(F) * wu[:, None]) / den[:, None] + F(0.5), F(0)), F(255)).astype(np.uint8)
    kc = keep & smp["has_color"]
    out = dict(sdf=np.where(keep, sdf, state["sdf"]), weight=np.where(keep, w_new, w_old), color=np.where(kc[:, None], col, state["color"]))
    out["sdf"] = np.where(reset, F(0), out["sdf"]); out["weight"] = np.where(reset, F(0), out["weight"]); out["color"] = np.where(reset[:, None], np.uint8(0), out["color"])
    return out


def reintegrate(state, smp_old, smp_new, first_frame, ordinal):
    """k_reintegrate per slot: subtract, reset rule, then add (first_frame already holds the new ordinal for the cells the new pose allocated)"""
    return integrate(deintegrate(state, smp_old, first_frame, ordinal), smp_new)


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------------------------------------
def pack(keys):
    k = np.asarray(keys, np.int64).reshape(-1, 3) + (1 << 20)
    return k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)


def lookup(export, keys):
    """the export's records at keys [n, 3]: dict(found, sdf, weight, color), zeros where the key is absent (as i3d_fusion_debug_voxels)"""
    have = pack(export["keys"]); want = pack(keys); n = want.shape[0]
    out = dict(found=np.zeros(n, bool), sdf=np.zeros(n, F), weight=np.zeros(n, F), color=np.zeros((n, 3), np.uint8))
    if have.size:
        order = np.argsort(have); pos = np.minimum(np.searchsorted(have[order], want), have.size - 1); idx = order[pos]
        hit = have[idx] == want
        out["found"] = hit
        for k in ("sdf", "weight", "color"):
            out[k][hit] = export[k][idx[hit]]
    return out


def first_frames(exports, keys):
    """index of the first per-frame export (the raw volume after frame 0, 1, ...) that holds each key; len(exports) where none does"""
    first = np.full(np.asarray(keys).reshape(-1, 3).shape[0], len(exports), np.int64)
    for i in range(len(exports) - 1, -1, -1):
        first[lookup(exports[i], keys)["found"]] = i
    return first


def union_keys(*key_sets):
    k = np.concatenate([np.asarray(a, np.int32).reshape(-1, 3) for a in key_sets])
    _, idx = np.unique(pack(k), return_index=True)
    return np.ascontiguousarray(k[np.sort(idx)])


# ---- the bounds of section 23.3 ----------------------------------------------------------------------------------------------------------------------------
def bounds(before, after, sample, frames):
    """per voxel: |d sdf| <= 8 eps (w_before / w_after) M with M the largest of |sdf before|, |sdf after|, |sample|;  |d w| <= 4 eps w_before;  colour per
    channel <= frames (w_before / w_after) + 1.  Four roundings in integrate and four in the inverse, each at most half an ulp of terms no larger than w_before M,
    divided by w_after, doubled because the later frames re-round on a different base; one truncation of less than a level per integrate, amplified by the same
    quotient, plus the final rounding."""
    wb = before["weight"].astype(np.float64); wa = after["weight"].astype(np.float64)
    q = wb / np.where(wa > 0, wa, 1.0)
    m = np.maximum(np.maximum(np.abs(before["sdf"]), np.abs(after["sdf"])), np.abs(sample)).astype(np.float64)
    return dict(sdf=8.0 * EPS * q * m, weight=4.0 * EPS * wb, color=frames * q + 1.0)
