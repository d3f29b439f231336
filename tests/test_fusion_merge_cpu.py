"""-m "not gpu": the numpy statement of i3d_fusion_merge (fusion_merge_twin.py) on hand-made volumes of a few dozen voxels: the aligned merge
is the per-voxel weighted mean, a lattice translation moves keys by m (negative coordinates included), the 8-candidate set of the allocation is the brute-force
scan of the bounding box under an oblique rotation, and an empty source changes nothing."""

import numpy as np

import fusion_deintegrate_twin as DT
import fusion_merge_twin as MT
from intrinsic3d_amd import synthetic

F = np.float32
VS = 0.0078125


def _block(lo, dim, seed, holes=0, zero_weight=0, first=0):
    """a dense block of voxels at lo with random sdf / weight / colour; `holes` of them absent, `zero_weight` stored with weight 0"""
    rng = np.random.default_rng(seed)
    k = np.stack(np.meshgrid(*[np.arange(lo[a], lo[a] + dim[a]) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    k = k[rng.permutation(len(k))[holes:]]
    n = len(k)
    w = rng.uniform(3.0, 20.0, n).astype(F); w[:zero_weight] = 0
    s = rng.uniform(-0.03, 0.03, n).astype(F); s[:zero_weight] = 0
    c = rng.integers(0, 256, (n, 3)).astype(np.uint8); c[:zero_weight] = 0
    return MT.volume(k, s, w, c, np.full(n, first))


def _by_key(v):
    return {tuple(int(x) for x in k): i for i, k in enumerate(v["keys"])}


def test_aligned_merge_is_the_weighted_mean():
    a = _block((-2, 0, 1), (4, 3, 3), 1, holes=5, zero_weight=3); b = _block((0, 1, 0), (4, 3, 3), 2, holes=4, zero_weight=2)
    out, st = MT.merge(a, b, VS, 7, m=(0, 0, 0))
    ia, ib, io = _by_key(a), _by_key(b), _by_key(out)
    fed = {k for k, i in ib.items() if b["weight"][i] != 0}
    assert set(io) == set(ia) | fed and len(io) == len(out["keys"])
    assert st == dict(ordinal=7, source_voxels=len(fed), sampled=len(fed), allocated=len(fed - set(ia)), aligned=1) and st["allocated"] > 0
    for k, o in io.items():
        s0, w0, c0 = (a["sdf"][ia[k]], a["weight"][ia[k]], a["color"][ia[k]]) if k in ia else (F(0), F(0), np.zeros(3, np.uint8))
        if k in fed:
            s1, w1, c1 = b["sdf"][ib[k]], b["weight"][ib[k]], b["color"][ib[k]]
            wn = F(w0 + w1)
            assert out["weight"][o] == wn and out["sdf"][o] == F(F(F(s0 * w0) + F(s1 * w1)) / wn)
            assert all(out["color"][o][ch] == np.uint8(F(F(F(F(c0[ch]) * w0) + F(F(c1[ch]) * w1)) / wn)) for ch in range(3))
        else:
            assert out["weight"][o] == w0 and out["sdf"][o] == s0 and (out["color"][o] == c0).all()
        assert out["first_frame"][o] == (a["first_frame"][ia[k]] if k in ia else 7)
    new = out["keys"][len(a["keys"]):]
    assert np.all(np.diff(DT.pack(new)) > 0)                                    # the inserted voxels in ascending order of packed key: their rank order


def test_lattice_translation_moves_keys_by_m():
    b = _block((-3, -2, -4), (5, 4, 4), 3, holes=6, zero_weight=4)
    m = np.array([-7, 3, -2])
    ok, mm = MT.aligned_of(np.concatenate([np.zeros(3), m * VS]), VS)
    assert ok and np.array_equal(mm, m)
    assert not MT.aligned_of(np.concatenate([np.zeros(3), m * VS + [0.0, 1e-4, 0.0]]), VS)[0]
    assert not MT.aligned_of(np.concatenate([[0.0, 1e-3, 0.0], m * VS]), VS)[0]
    assert MT.aligned_of(None, VS)[0]
    out, st = MT.merge(MT.volume(), b, VS, 0, m=mm)
    on = b["weight"] != 0
    assert st["allocated"] == st["sampled"] == int(on.sum()) and (out["keys"] < 0).any()
    want = b["keys"][on] + m
    order = np.argsort(DT.pack(want))
    assert np.array_equal(out["keys"], want[order]) and np.array_equal(out["weight"], b["weight"][on][order])
    assert np.array_equal(out["sdf"], (b["sdf"][on][order] * b["weight"][on][order]) / b["weight"][on][order])
    w = b["weight"][on][order][:, None]; c = b["color"][on][order]
    assert np.array_equal(out["color"], ((c.astype(F) * w) / w).astype(np.uint8))  # sample_add truncates: where (c w) / w rounds below c the channel loses a level,
    assert np.all(c.astype(int) - out["color"] <= 1) and np.all(out["color"] <= c)  # as it does for a frame's first sample


def test_candidate_set_is_the_brute_force_scan():
    b = _block((-3, 2, -1), (6, 5, 5), 4, holes=12, zero_weight=6)
    axis = np.array([0.3, -0.8, 0.52]); aa = axis / np.linalg.norm(axis) * np.radians(20.0)
    R = synthetic.aa_to_rotmat(aa); t = np.array([0.0131, -0.0207, 0.0049]); tv = t / VS
    img = (b["keys"].astype(np.float64) @ R.T) + tv
    lo, hi = np.floor(img.min(0)).astype(int) - 3, np.ceil(img.max(0)).astype(int) + 4
    box = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a]) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    brute = box[MT.sample_general(b, VS, R, t, box)["on"]]
    cand = MT.candidates(b, R, tv)
    fed = cand[MT.sample_general(b, VS, R, t, cand)["on"]]
    assert len(brute) > 20 and set(map(tuple, brute)) == set(map(tuple, fed))
    out, st = MT.merge(MT.volume(), b, VS, 2, R=R, t=t, tv=tv)
    assert st["allocated"] == st["sampled"] == len(brute) and set(map(tuple, out["keys"])) == set(map(tuple, brute))
    # a trilinear sample lies within its corners' range, and the weight of an empty voxel is the sample's
    smp = MT.sample_general(b, VS, R, t, out["keys"])
    assert np.array_equal(out["weight"], smp["wu"]) and np.all(smp["wu"] >= 3.0 * (1 - 1e-6)) and np.all(np.abs(smp["sample"]) <= 0.03)


def test_empty_source_changes_nothing():
    a = _block((0, 0, 0), (3, 3, 3), 5, zero_weight=2)
    dead = MT.volume(a["keys"] + 1, np.zeros(len(a["keys"]), F), np.zeros(len(a["keys"]), F))      # stored, but nothing has a weight
    for src in (MT.volume(), dead):
        for kw in (dict(m=(1, -1, 0)), dict(R=np.eye(3), t=np.array([0.001, 0.0, 0.0]), tv=np.array([0.128, 0.0, 0.0]))):
            out, st = MT.merge(a, src, VS, 3, **kw)
            assert st["source_voxels"] == st["sampled"] == st["allocated"] == 0
            for k in ("keys", "sdf", "weight", "color", "first_frame"):
                assert np.array_equal(out[k], a[k]), k
