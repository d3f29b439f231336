"""-m gpu: the device stages of i3d_estimate_sh (k_sh_all_keys / k_sh_keys, the sorts, k_sh_assign, k_sh_gram on the fp64 matrix cores, k_sh_gram_sum,
k_sh_interpolate) against their numpy statement tests/sh_twin.py, stage by stage, on the grids of tests/sh_cases.py.  The twin is pinned
against the oracle by tests/test_sh_twin_cpu.py, which also shows that the Gram bound used here is broken by a dropped voxel, a doubled one, a zeroed weight, two
swapped feature slots, an fp32 accumulation and two exchanged runs.

Measured on an MI355X: Gram error / bound 0.0001 .. 0.018, weight-sum error / bound 0 .. 0.049, no interpolated value different from
the twin's; on the awkward cases k_sh_interpolate follows the single-rounded p (the compiler fuses the multiply into the subtraction)."""
import threading

import numpy as np
import pytest

import sh_cases
import sh_twin

pytestmark = pytest.mark.gpu
F = np.float32
CASES = ["runs0", "runs1", "single", "ineligible", "awkward0.05", "awkward0.035"]
EXACT_SUBVOLUME_ARITHMETIC = ["runs0", "runs1", "single", "ineligible"]          # voxel size and subvolume size are powers of two: both roundings of p coincide
LAMBDA = 10.0


def _case(name):
    return {c["name"]: c for c in sh_cases.all_cases()}[name]


def _context(name):
    from intrinsic3d_amd import binding
    g = _case(name)["grid"]
    ctx = binding.Context(0)
    ctx.set_grid(g["voxel_size"], g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
    return ctx


@pytest.fixture(scope="module")
def device():
    """case name -> (context holding the case's grid, what debug_sh_stages returned): one context and one debug call per case, shared by the tests"""
    cache = {}

    def get(name):
        if name not in cache:
            c = _case(name); ctx = _context(name)
            cache[name] = (ctx, ctx.debug_sh_stages(c["size"], c["thres"]))
        return cache[name]
    yield get
    for ctx, _ in cache.values():
        ctx.close()


def _gram_ratio(dev, st):
    """largest |G_dev - G_twin| / bound over the entries with a bound > 0; the entries without (empty subvolumes) must be exact zeros"""
    bound = sh_twin.gram_bound(st["A"], st["n"]); err = np.abs(dev["gram"] - st["gram"])
    assert np.all(dev["gram"][bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def _weight_ratio(dev, st):
    bound = sh_twin.weight_bound(st["weight_sum"], st["n"]); err = np.abs(dev["weight_sum"] - st["weight_sum"])
    assert np.all(dev["weight_sum"][bound == 0] == 0)
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("name", CASES)
def test_discrete_outputs_equal_the_twin(device, name):
    """the subvolume set and its order, and every voxel's subvolume or -1: no tolerance, no share of flips"""
    _, dev = device(name); st = sh_cases.twin_stages(name)
    assert dev["indices"].shape[0] == st["indices"].shape[0]
    assert np.array_equal(dev["indices"], st["indices"])
    assert np.array_equal(dev["voxel_subvolume"], st["voxel_subvolume"]), np.nonzero(dev["voxel_subvolume"] != st["voxel_subvolume"])[0][:10]
    got = dev["voxel_subvolume"][dev["voxel_subvolume"] >= 0]
    assert np.array_equal(np.bincount(got, minlength=len(st["n"])), st["n"])                         # the run lengths


@pytest.mark.parametrize("name", CASES)
def test_gram_blocks_within_fp64_round_off(device, name):
    """|G_dev - G_twin| <= 4 (n_s + 32) 2^-53 A entry by entry (sh_twin.gram_bound), all 100 entries: G[i][j] and G[j][i] each meet it.  The blocks and weight
    sums of empty subvolumes are exactly 0."""
    _, dev = device(name); st = sh_cases.twin_stages(name)
    ratio = _gram_ratio(dev, st)
    print(f"\n{name}: largest Gram error / bound = {ratio:.4f} (S = {len(st['n'])}, longest run {int(st['n'].max())})")
    empty = st["n"] == 0
    assert np.all(dev["gram"][empty] == 0) and np.all(dev["weight_sum"][empty] == 0)
    assert ratio <= 1.0


@pytest.mark.parametrize("name", CASES)
def test_weight_sums_within_fp64_round_off(device, name):
    """|w_dev - w_twin| <= (n_s + 8) 2^-53 w_twin"""
    _, dev = device(name); st = sh_cases.twin_stages(name)
    ratio = _weight_ratio(dev, st)
    print(f"\n{name}: largest weight-sum error / bound = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", ["runs0", "runs1", "single"])
def test_one_chunk_per_launch_gives_the_same_bits(device, monkeypatch, name):
    ctx, dev = device(name); c = _case(name)
    monkeypatch.setenv("I3D_SH_SLAB", "1")
    slab = ctx.debug_sh_stages(c["size"], c["thres"])
    monkeypatch.delenv("I3D_SH_SLAB")
    assert sh_cases.twin_stages(name)["n"].max() > 2048                                               # several chunks, so several launches
    assert np.array_equal(slab["gram"].view(np.uint64), dev["gram"].view(np.uint64))
    assert np.array_equal(slab["weight_sum"].view(np.uint64), dev["weight_sum"].view(np.uint64))
    assert np.array_equal(slab["voxel_subvolume"], dev["voxel_subvolume"])


def _ordered(a):
    """fp32 bit patterns as integers in the order of the values: the difference of two is their distance in ulps"""
    i = np.ascontiguousarray(a, F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _ulp_report(got, want):
    d = np.abs(_ordered(got) - _ordered(want))
    return int(d.max()), int((d != 0).sum())


@pytest.mark.parametrize("name", CASES)
def test_interpolation_and_stats(device, name):
    """After estimate_sh, get_voxel_sh() against sh_twin.interpolate of the coefficients and indices the call returned: every value equal or one fp32 ulp apart,
    at most 1e-4 of the values different at all (fp64 fused against separate accumulation), against ONE rounding of p for all voxels and axes; exact zeros
    outside the shell and at weight 0; in the single-volume case the cast coefficients everywhere in the shell.  The stats are the twin's counts."""
    ctx, _ = device(name); c = _case(name); g = c["grid"]; st = sh_cases.twin_stages(name)
    sh, idx, stats = ctx.estimate_sh(c["size"], LAMBDA, c["thres"])
    assert stats.subvolumes == len(st["indices"]) and stats.data_rows == int((st["voxel_subvolume"] >= 0).sum()) and stats.reg_rows == len(st["pairs"])
    assert np.array_equal(idx, st["indices"])
    v64 = ctx.get_voxel_sh(); got = v64.astype(F)
    assert np.array_equal(got.astype(np.float64), v64)
    shell = sh_twin.in_shell(g, c["thres"])
    assert np.all(got[~shell] == 0) and not shell[g["weight"] <= 0].any()
    variants = {"separate": sh_twin.interpolate(g["keys"], g["voxel_size"], c["size"], idx, sh, shell, fused=False),
                "single-rounded": sh_twin.interpolate(g["keys"], g["voxel_size"], c["size"], idx, sh, shell, fused=True)}
    if name in EXACT_SUBVOLUME_ARITHMETIC:
        assert np.array_equal(variants["separate"].view(np.uint32), variants["single-rounded"].view(np.uint32))
    if c["size"] <= 0:
        assert np.array_equal(got[shell].view(np.uint32), np.broadcast_to(sh[0].astype(F), got[shell].shape).copy().view(np.uint32))
    report = {k: _ulp_report(got, w) for k, w in variants.items()}
    ok = [k for k, (worst, differing) in report.items() if worst <= 1 and differing <= 1e-4 * got.size]
    print(f"\n{name}: interpolation against the twin, (largest distance in ulps, values that differ) of {got.size}: {report}; the kernel follows: {ok}")
    assert ok, report


def test_debug_call_leaves_the_lighting_state_alone(device):
    """estimate, debug (with another subvolume size), estimate: the same bits from both estimates, and the per-voxel SH untouched in between"""
    ctx, _ = device("awkward0.035"); c = _case("awkward0.035")
    a = ctx.estimate_sh(c["size"], LAMBDA, c["thres"]); va = ctx.get_voxel_sh()
    ctx.debug_sh_stages(0.05, c["thres"]); ctx.debug_sh_stages(0.0, c["thres"])
    vb = ctx.get_voxel_sh()
    b = ctx.estimate_sh(c["size"], LAMBDA, c["thres"]); vc = ctx.get_voxel_sh()
    assert np.array_equal(va.view(np.uint64), vb.view(np.uint64)) and np.array_equal(va.view(np.uint64), vc.view(np.uint64)) and np.abs(va).max() > 0
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])
    for f in ("data_rows", "reg_rows", "subvolumes", "lm_iterations", "termination", "cost_initial", "cost_final"):
        assert getattr(a[2], f) == getattr(b[2], f), f


def test_debug_call_does_not_make_the_context_shadeable():
    from intrinsic3d_amd import binding
    ctx = _context("ineligible"); c = _case("ineligible")
    cam = dict(width=8, height=8, intr=(10.0, 10.0, 4.0, 4.0), pose=np.zeros(6))
    try:
        for _ in range(2):                                    # before and after the debug call: the same refusal
            with pytest.raises(binding.I3DError, match=r"\(4\).*per-voxel SH"):
                ctx.render_view(frame=-1, planes=("shading",), camera=cam)
            ctx.debug_sh_stages(c["size"], c["thres"])
    finally:
        ctx.close()


def test_two_simulated_ranks_share_one_sum(device):
    """Two ranks (host threads on one device): each accumulates its half of the sorted list, the all-reduce hands both the same blocks.  The cut M / 2 falls inside
    a run and not on a chunk boundary, so one run's blocks are the sum of two ranks' partial chunks."""
    from intrinsic3d_amd import binding
    name = "runs0"; c = _case(name); st = sh_cases.twin_stages(name)
    n = st["n"]; M = int(n.sum()); cut = M // 2; starts = np.concatenate([[0], np.cumsum(n)])
    s = int(np.searchsorted(starts, cut, side="right") - 1)
    assert starts[s] < cut < starts[s + 1] and (cut - starts[s]) % 2048 != 0
    L = binding.load(); shared = L.i3d_comm_sim_create(2)
    ctxs = [_context(name) for _ in range(2)]
    out = [None, None]; err = [None, None]
    try:
        for r, ctx in enumerate(ctxs):
            ctx.comm_init_sim(shared, r)

        def run(r):
            try:
                out[r] = ctxs[r].debug_sh_stages(c["size"], c["thres"])
            except Exception as e:      # surface a failure instead of leaving the other rank waiting silently
                err[r] = e
        th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
        [t.start() for t in th]; [t.join(timeout=120) for t in th]
        assert not any(t.is_alive() for t in th), "sharded run hung"
        assert all(e is None for e in err), err
        for k in ("gram", "weight_sum"):
            assert np.array_equal(out[0][k].view(np.uint64), out[1][k].view(np.uint64)), k
        for k in ("indices", "voxel_subvolume"):
            assert np.array_equal(out[0][k], st[k]) and np.array_equal(out[1][k], st[k]), k
        ratio = _gram_ratio(out[0], st); wratio = _weight_ratio(out[0], st)
        print(f"\n{name}, two ranks: largest Gram error / bound = {ratio:.4f}, weight-sum error / bound = {wratio:.4f}")
        assert ratio <= 1.0 and wratio <= 1.0
    finally:
        for ctx in ctxs:
            ctx.close()
        L.i3d_comm_sim_destroy(shared)


def test_errors(device):
    from intrinsic3d_amd import binding
    ctx = binding.Context(0)
    try:
        with pytest.raises(binding.I3DError, match=r"\(4\).*no grid"):
            ctx.debug_sh_stages(0.05, 0.008)
    finally:
        ctx.close()
    ctx, _ = device("runs0"); c = _case("runs0")
    for thres in (0.0, -1.0):
        with pytest.raises(binding.I3DError, match=r"\(1\).*thres_shell"):
            ctx.debug_sh_stages(c["size"], thres)
    with pytest.raises(binding.I3DError, match=r"\(5\).*capacity"):
        ctx.debug_sh_stages(c["size"], c["thres"], cap=5)                                             # S = 6
    assert ctx.debug_sh_stages(c["size"], c["thres"], cap=6)["indices"].shape[0] == 6
    assert binding.load().i3d_debug_sh_stages(None, 0.05, 0.008, 8, None, None, None, None, None) == 1
