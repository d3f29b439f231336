"""No GPU: tests/sh_twin.py is pinned here before tests/test_gpu_sh_stages.py lets it judge the device.

1. the cases of tests/sh_cases.py hold what they were built to hold (exactness conditions, run lengths, the awkward floors and missing corners);
2. against the oracle: subvolume set, row counts, the mask of voxels that receive coefficients, the interpolation bit for bit, and the minimiser of the twin's
   normal equations against the oracle's coefficients;
3. the Gram bound has teeth: six defects a kernel could have, applied to the twin's inputs, each break it on the "runs" grid."""
import numpy as np
import pytest

import sh_cases
import sh_twin

F = np.float32
ORACLE_CASES = ["runs0", "runs1", "ineligible", "awkward0.05", "awkward0.035"]


def _case(name):
    return {c["name"]: c for c in sh_cases.all_cases()}[name]


# ---- 1. the cases -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["runs0", "runs1", "single"])
def test_exactness_conditions(name):
    """The fp32 expressions of the features, evaluated in fp64, give the fp32 results: no rounding happens where a fused multiply-add could round differently."""
    c = _case(name); g = c["grid"]
    assert F(g["voxel_size"]) == 2.0 ** -8 and c["thres"] == 2.0 * g["voxel_size"] == 64 * sh_cases.Q
    k = g["sdf_refined"] / sh_cases.Q
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() <= 60
    assert np.array_equal(g["sdf_refined"].astype(F).astype(np.float64), g["sdf_refined"])
    nb = sh_twin.neighbours(g); el = sh_twin.eligible(g, c["thres"], nb)
    d32, len32 = sh_twin.forward_differences(g, nb)
    d32 = d32[el]; f64 = g["sdf_refined"]
    d64 = np.stack([f64[nb[el, a]] - f64[el] for a in range(3)], axis=1)
    assert np.array_equal(d32.astype(np.float64), d64)                                              # differences
    sq64 = d64 * d64
    assert np.array_equal((d32 * d32).astype(np.float64), sq64)                                     # squares
    s64 = sq64[:, 0] + (sq64[:, 1] + sq64[:, 2])
    assert np.array_equal(s64.astype(F).astype(np.float64), s64) and np.all(s64 / sh_cases.Q ** 2 < 2 ** 24)      # the sums, in any order, fused or not
    assert np.array_equal(len32[el], np.sqrt(s64).astype(F))                                        # sqrt of an exact fp32 value: correctly rounded either way
    assert np.all((g["color"] != 0).sum(axis=1) == 1)                                               # the luminance is one product and one quotient
    assert g["albedo"][el].min() >= 0.3 and g["albedo"][el].max() <= 1.0
    if c["size"] > 0:                                                                                 # and the subvolume arithmetic is exact as well
        assert np.array_equal(sh_twin.subvolume_index(g["keys"], g["voxel_size"], c["size"]), np.floor_divide(g["keys"], 32))
    f, _ = sh_twin.features(g, el, nb)
    assert np.unique(f[:, 1:9], axis=0).shape[0] == f.shape[0]                                      # distinct feature vectors: a mixed-up slot cannot cancel


@pytest.mark.parametrize("arrangement", [0, 1])
def test_run_lengths_are_the_ones_asked_for(arrangement):
    c = sh_cases.runs(arrangement); st = sh_cases.twin_stages(c["name"])
    assert st["indices"].tolist() == [[x, -1, -1] for x in range(-3, 3)] and len(st["indices"]) % 4 == 2
    assert st["n"].tolist() == list(c["run_lengths"])
    assert np.array_equal(np.bincount(st["voxel_subvolume"][st["voxel_subvolume"] >= 0], minlength=6), st["n"])


def test_run_lengths_cover_every_edge():
    have = set(sh_cases.RUN_LENGTHS[0]) | set(sh_cases.RUN_LENGTHS[1])
    assert have >= {0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097}
    for a in sh_cases.RUN_LENGTHS:                                                                   # a stored but empty subvolume between two non-empty ones
        i = a.index(0); assert 0 < i < 5 and a[i - 1] > 0 and a[i + 1] > 0


def test_single_is_one_run_with_a_partial_last_tile():
    st = sh_cases.twin_stages("single")
    n = int(st["n"][0])
    assert st["indices"].tolist() == [[0, 0, 0]] and n == sum(sh_cases.RUN_LENGTHS[0]) and n > 4 * 2048 and n % 2048 > 64 and n % 64 != 0
    assert np.array_equal(st["voxel_subvolume"] >= 0, sh_cases.twin_stages("runs0")["voxel_subvolume"] >= 0)


def test_ineligible_probes():
    c = sh_cases.ineligible(); g = c["grid"]; st = sh_cases.twin_stages("ineligible")
    pos = {tuple(k): i for i, k in enumerate(g["keys"].tolist())}
    el = st["voxel_subvolume"] >= 0
    for what, t in c["probes"].items():
        assert el[pos[t]] == (what == "at_thres"), what
        ring = [pos.get(tuple(np.add(t, d))) for d in sh_twin.RING6]
        assert any(r is not None and el[r] for r in ring), what                                     # the defect stays with its probe: a voxel beside it passes
    assert (pos[c["probes"]["weight0"]] is not None) and g["weight"][pos[c["probes"]["weight0"]]] == 0
    t = c["probes"]["missing_py"]; assert (t[0], t[1] + 1, t[2]) not in pos
    assert np.signbit(g["albedo"][pos[c["probes"]["albedo_negative_zero"]]])


def test_awkward_holds_what_it_was_built_for():
    tails = []; near = []; missing = []
    for size in sh_cases.AWKWARD_SIZES:
        c = sh_cases.awkward(size); g = c["grid"]; st = sh_cases.twin_stages(c["name"])
        for a in range(3):
            assert g["keys"][:, a].min() < 0 < g["keys"][:, a].max() and st["indices"][:, a].min() < 0 <= st["indices"][:, a].max()
        tails.append(len(st["indices"]) % 4)
        shell = sh_twin.in_shell(g, c["thres"])
        ids, w8 = sh_twin.corner_lookup(g["keys"], g["voxel_size"], size, st["indices"])
        missing.append(int(((ids[shell] < 0) & (w8[shell] != 0)).any(axis=1).sum()))
        v = (g["keys"].astype(F) * F(g["voxel_size"])) * (F(1.0) / F(size))
        m = (g["keys"] != 0) & (np.abs(v - np.rint(v)) <= 2 * np.spacing(np.abs(np.rint(v)).astype(F)))
        near.append(int(m.sum()))
    assert any(tails), tails                      # S % 4 != 0
    assert all(missing), missing                  # in-shell voxels with a missing corner subvolume that carries weight
    assert any(near), near                        # a non-zero key whose (float(c) * vs) * inv lies within 2 ulp of an integer


# ---- 2. against the oracle ----------------------------------------------------------------------------------------------------------------------------------

LAMBDA = 10.0
# max |oracle - minimiser| / max |minimiser| over the coefficients, as measured (the oracle's Ceres-style LM stops on a relative cost change of 1e-6, so this
# distance is set by its stopping rule and cannot be derived); the test allows ten times as much
ORACLE_DISTANCE = {"runs0": 3.085e-4, "runs1": 2.249e-3, "ineligible": 8.287e-3, "awkward0.05": 1.471e-3, "awkward0.035": 1.405e-4}


@pytest.fixture(scope="module")
def on_oracle(oracle):
    """case name -> (the grid in the oracle's visit order, the oracle's estimate), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = _case(name); g = c["grid"]
            og = oracle.Grid.from_voxels(g["voxel_size"], g["keys"], g["sdf"], g["weight"], g["color"])        # drops the voxels of weight 0
            ok = og.export()["keys"]
            pos = {tuple(k): i for i, k in enumerate(g["keys"].tolist())}
            order = np.array([pos[tuple(k)] for k in ok.tolist()])
            assert sorted(order.tolist()) == np.nonzero(g["weight"] > 0)[0].tolist()
            og.import_fields(sdf_refined=g["sdf_refined"][order], albedo=g["albedo"][order])
            rc, sh, idx, vsh, has, st = oracle.estimate_sh(og, c["size"], LAMBDA, c["thres"])
            assert rc == 0
            og.free()
            cache[name] = dict(order=order, sh=sh, idx=idx, vsh=vsh, has=has.astype(bool), st=st)
        return cache[name]
    return get


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_discrete_outputs_match_the_oracle(on_oracle, name):
    c = _case(name); g = c["grid"]; st = sh_cases.twin_stages(name); o = on_oracle(name)
    # the oracle lists its subvolumes in the order of its hash map, which means nothing; the device's order is the packed one, and the twin's must be that
    assert np.all(np.diff(sh_twin.pack(st["indices"])) > 0)
    assert sorted(map(tuple, o["idx"].tolist())) == sorted(map(tuple, st["indices"].tolist()))
    assert o["st"].subvolumes == len(st["indices"])
    assert o["st"].data_rows == int((st["voxel_subvolume"] >= 0).sum()) == int(st["n"].sum())
    assert o["st"].reg_rows == len(st["pairs"])
    shell = sh_twin.in_shell(g, c["thres"])
    assert np.array_equal(o["has"], shell[o["order"]])
    assert not shell[g["weight"] <= 0].any()


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_interpolation_matches_the_oracle_bit_for_bit(on_oracle, name):
    """the separate-rounding variant of the twin, on the oracle's own coefficients and subvolume order, against the oracle's per-voxel coefficients cast to fp32"""
    c = _case(name); g = c["grid"]; o = on_oracle(name)
    got = sh_twin.interpolate(g["keys"][o["order"]], g["voxel_size"], c["size"], o["idx"], o["sh"], o["has"], fused=False)
    want = o["vsh"].astype(F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    assert np.all(got[~o["has"]] == 0) and o["has"].sum() > 0 and np.abs(got[o["has"]]).max() > 0


def _constant(st):
    """the part of the cost that does not depend on the coefficients: sum w I^2 / (2 sum w)"""
    return 0.5 * st["gram"][:, 9, 9].sum() / st["weight_sum"].sum()


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_minimiser_of_the_twins_normal_equations_is_where_the_oracle_stops(on_oracle, name):
    st = sh_cases.twin_stages(name); o = on_oracle(name)
    x, H, b = sh_twin.minimiser(st["gram"], st["weight_sum"], st["pairs"], LAMBDA)
    look = {tuple(k): i for i, k in enumerate(o["idx"].tolist())}
    osh = o["sh"][[look[tuple(k)] for k in st["indices"].tolist()]]
    dist = np.abs(osh - x).max() / np.abs(x).max()
    grad = np.abs(H @ osh.ravel() - b).max() / np.abs(b).max()
    print(f"{name}: oracle to exact minimiser {dist:.3e} of the largest coefficient ({np.abs(x).max():.3f}); relative gradient left {grad:.3e}")
    assert dist <= 10.0 * ORACLE_DISTANCE[name]
    # what the stopping rule does not blur: the oracle's own cost at its start (zero coefficients) and at the point where it stopped, from the twin's blocks
    xo = osh.ravel()
    assert o["st"].cost_initial == pytest.approx(_constant(st), rel=1e-11)
    assert o["st"].cost_final == pytest.approx(0.5 * xo @ H @ xo - b @ xo + _constant(st), rel=1e-9)


# ---- 3. the bound has teeth ---------------------------------------------------------------------------------------------------------------------------------

def _runs0_inputs():
    st = sh_cases.twin_stages("runs0")
    sub = st["voxel_subvolume"][st["voxel_subvolume"] >= 0]
    return st, st["features"], st["weights"], sub


def _breaks(st, G, ws=None):
    over = np.abs(G - st["gram"]) > sh_twin.gram_bound(st["A"], st["n"])
    return bool(over.any())


def test_plain_fp64_accumulation_meets_the_bound():
    """the control: an honest fp64 sum of the same terms, in list order, is inside the bound the mutations break"""
    st, f, w, sub = _runs0_inputs()
    G = np.zeros_like(st["gram"])
    for s in range(6):
        m = sub == s
        for v in np.nonzero(m)[0]:
            G[s] += np.outer(w[v] * f[v], f[v])
    ratio = np.abs(G - st["gram"]) / np.where(st["A"] > 0, sh_twin.gram_bound(st["A"], st["n"]), 1.0)
    assert ratio.max() < 0.25 and not _breaks(st, G)
    assert np.all(st["gram"][2] == 0) and st["weight_sum"][2] == 0                                   # the empty subvolume


def _member(sub, s, position):
    return np.nonzero(sub == s)[0][position]


MUTATIONS = ["drop_last_of_longest_run", "count_position_64_twice", "zero_weight_in_tail_tile", "swap_two_feature_slots", "accumulate_in_fp32",
             "exchange_two_neighbouring_runs"]


@pytest.mark.parametrize("what", MUTATIONS)
def test_mutation_breaks_the_gram_bound(what):
    st, f, w, sub = _runs0_inputs()
    f = f.copy(); w = w.copy(); sub = sub.copy(); fp32 = False
    longest = int(np.argmax(st["n"])); assert st["n"][longest] == 4097
    if what == "drop_last_of_longest_run":
        keep = np.ones(len(w), bool); keep[_member(sub, longest, -1)] = False
        f, w, sub = f[keep], w[keep], sub[keep]
    elif what == "count_position_64_twice":
        v = _member(sub, longest, 64)
        f = np.concatenate([f, f[v:v + 1]]); w = np.concatenate([w, w[v:v + 1]]); sub = np.concatenate([sub, sub[v:v + 1]])
    elif what == "zero_weight_in_tail_tile":
        assert st["n"][0] == 2049
        w[_member(sub, 0, 2048)] = 0.0                                                                # the one voxel of the tile after a full chunk
    elif what == "swap_two_feature_slots":
        v = _member(sub, longest, 1000); f[v, [1, 2]] = f[v, [2, 1]]
    elif what == "accumulate_in_fp32":
        fp32 = True
    elif what == "exchange_two_neighbouring_runs":
        a, b = sub == 3, sub == 4; sub[a] = 4; sub[b] = 3
    G, ws, _, _ = sh_twin.gram(f, w, sub, 6, fp32=fp32)
    assert _breaks(st, G), what
