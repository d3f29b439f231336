"""-m gpu: the device's trust-region controller (lm_kernels.hip: k_lm_init, k_lm_begin, k_lm_begin_lad, k_lm_decide), branch by branch.

i3d_debug_lm_script runs these kernels alone, through the launches of lm_solve and in its order, on a SCRIPT of attempt outcomes (what the PCG solve, the candidate
and the cost pass would have left on the device).  Each script is a few dozen scalars.  Checked:

  * against tests/lm_controller_twin.py (written from SURVEY.md B.2 and the two Ceres rules it cites), record by record: the integer fields equal, the fp64 fields
    bit for bit - they are IEEE + - * / sqrt min max - except the radius after an ACCEPTED step, which goes through pow: within 8 ulp (pow <= 2 ulp; 1 - p amplifies
    the error of p by p / (1 - p) <= 2 where the max(1/3, .) clip does not take over; one division and one min follow);
  * the ladder (every batch plan) against the serial loop: the records of kind 0 / 1 / 2 bit for bit, as many kind-3 records as the twin predicts, the radius of every
    system as the twin sets the batch up, a decided attempt's system at the radius the serial loop holds there, dead systems with inv_radius 0 and nothing written;
  * the block-Jacobi setup against the twin's numpy.linalg.inv, the LM diagonal of the camera tail against numpy.float32, the ladder's against the serial loop's at the
    same radius bit for bit, and the floats around every output range untouched, at K = 1, 63, 64, 65, 130 (the 64-thread block tails).
The module prints the largest ulp distance of an accepted radius, the largest block-inverse error against its bound and the resync counts per batch plan."""
import numpy as np
import pytest

import lm_controller_twin as T

pytestmark = pytest.mark.gpu

PLANS = [(2,), (4,), (6,), (1, 3, 2, 6)]
G = 64


@pytest.fixture(scope="module")
def ctx():
    from intrinsic3d_amd import binding
    c = binding.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- scripts ----------------------------------------------------------------
COST = 10.0


def att(xbr=1.0, d2xx=1.0, it=7, done=1, step2=1.0, x2=4.0, cand=COST + 1.0, dbg=0):
    return {"xbr": xbr, "d2xx": d2xx, "it": it, "done": done, "step2": step2, "x2": x2, "cand": cand, "dbg": dbg}


def rej(**kw):                     # rho = -1
    return att(**kw)


def acc(rho=0.5, cost=COST, **kw):  # model_change = 1: cand = cost - rho
    return att(cand=cost - rho, **kw)


def inv(how="sign"):
    return {"sign": att(xbr=-3.0), "zero": att(xbr=-1.0), "nan_xbr": att(xbr=np.nan), "nan_d2": att(d2xx=np.nan), "pinf": att(xbr=np.inf), "ninf": att(d2xx=-np.inf),
            "inf_both": att(xbr=np.inf, d2xx=-np.inf), "flag": att(dbg=1)}[how]


def ptol():
    return att(step2=1e-20)        # |delta| = 1e-10 <= 1e-8 (2 + 1e-8)


def ftol():
    return att(cand=COST - 1e-7 * COST)


def script(name, attempts, expect, lm_steps=None, radius0=1e4, ngrad=3.0, nfree=100.0, cost=COST):
    """expect: the `what` of the twin's last record (the named branch), or a callable on the twin's records"""
    lm_steps = len(attempts) if lm_steps is None else lm_steps
    attempts = list(attempts) + [rej()] * max(0, lm_steps - len(attempts))
    return {"name": name, "attempts": attempts, "expect": expect, "lm_steps": lm_steps, "radius0": radius0, "ngrad": ngrad, "nfree": nfree, "cost": cost}


def whats(recs):
    return [r["what"] for r in recs]


SCRIPTS = [
    script("accept at 0", [acc()], "accept", lm_steps=5),
    script("accept at 1", [rej(), acc()], "accept", lm_steps=5),
    script("accept at 5", [rej()] * 5 + [acc()], "accept", lm_steps=50),
    script("ngrad 0", [rej()], "init", ngrad=0.0),
    script("nfree 0", [rej()], "init", nfree=0.0),
    script("five invalid", [inv("sign")] * 5, "invalid-fail", lm_steps=10),
    script("four invalid, rejected, five invalid", [inv("nan_xbr")] * 4 + [rej()] + [inv("flag")] * 5, lambda r: whats(r)[-1] == "invalid-fail" and len(r) == 11, lm_steps=20),
    script("four invalid, rejected, four invalid, accept", [inv("sign")] * 4 + [rej()] + [inv("zero")] * 4 + [acc()], lambda r: whats(r)[-1] == "accept" and len(r) == 11, lm_steps=20),
    script("pcg breakdown", [rej(it=3, done=2), acc(it=0, done=2)], lambda r: [x["pcg_it"] for x in r[1:]] == [4, 1], lm_steps=5),
    script("lm_steps 1", [rej()], "reject+limit"),
    script("lm_steps 3, all rejected", [rej()] * 3, "reject+limit"),
    script("lm_steps 5, all rejected", [rej()] * 5, "reject+limit"),
    script("lm_steps 5, invalid last", [rej()] * 4 + [inv("sign")], "invalid+limit"),
    script("radius0 1e-31", [rej()] * 8, lambda r: r[-1]["kind"] == 2 and len(r) == 5, radius0=1e-31),
    script("radius0 1e-33", [rej()] * 4, lambda r: r[-1]["kind"] == 2 and len(r) == 2, radius0=1e-33),
    script("radius0 1.5e-32, invalid first", [inv("sign")] + [rej()] * 4, lambda r: r[-1]["kind"] == 2 and len(r) == 3, radius0=1.5e-32),
    script("rejected until the radius runs out", [rej()] * 50, lambda r: r[-1]["kind"] == 2 and len(r) == 17),
    script("cap 1e16", [acc(1.0)], lambda r: r[-1]["radius_after"] == 1e16 and r[-1]["what"] == "accept-clip", lm_steps=3, radius0=5e15),
    script("below the cap", [acc(1.0)], lambda r: abs(r[-1]["radius_after"] - 3e15) < 1e3 and r[-1]["what"] == "accept-clip", lm_steps=3, radius0=1e15),
    script("rho 0.95: clip", [rej(), acc(0.95)], "accept-clip", lm_steps=4),
    script("rho 0.9: no clip", [rej(), acc(0.9)], "accept", lm_steps=4),
    script("rho 0.9368: just clipped", [acc(0.9368)], "accept-clip", lm_steps=4),
    script("rho 0.9367: just not", [acc(0.9367)], "accept", lm_steps=4),
    script("rho 0.3", [acc(0.3)], "accept", lm_steps=4),
    script("rho 0.0011", [acc(0.0011)], "accept", lm_steps=4),
    script("rho 0.0009", [acc(0.0009), acc(0.7)], lambda r: whats(r)[1:] == ["reject", "accept"], lm_steps=4),
    script("rho 7 (cost falls further than the model)", [acc(7.0)], "accept-clip", lm_steps=4),
    script("parameter tolerance at 0", [ptol()], "parameter-tolerance", lm_steps=4),
    script("parameter tolerance inside a batch", [rej(), rej(), ptol()], "parameter-tolerance", lm_steps=9),
    script("function tolerance at 0", [ftol()], "function-tolerance", lm_steps=4),
    script("function tolerance inside a batch", [rej(), rej(), rej(), ftol()], "function-tolerance", lm_steps=9),
    script("candidate cost NaN", [att(cand=np.nan), acc()], lambda r: whats(r)[1:] == ["reject", "accept"], lm_steps=4),
    script("candidate cost inf", [att(cand=np.inf), acc()], lambda r: whats(r)[1:] == ["reject", "accept"], lm_steps=4),
    script("62 attempts", ([inv("sign")] * 4 + [rej()]) * 13, lambda r: len(r) == 63 and r[-1]["what"].endswith("+limit"), lm_steps=62, radius0=1e16),
] + [script(f"invalid at 0 by {how}", [inv(how), rej(), rej(), acc()], "accept", lm_steps=9) for how in ("sign", "zero", "nan_xbr", "nan_d2", "pinf", "ninf", "inf_both", "flag")] \
  + [script("invalid at 1", [rej(), inv("flag"), rej(), rej(), acc()], "accept", lm_steps=9),
     script("invalid at 0, accept at 1", [inv("flag"), acc()], "accept", lm_steps=9)]


def twin_inputs(s):
    return [{"model_change": 0.5 * a["xbr"] + 0.5 * a["d2xx"], "step_norm2": a["step2"], "x_norm2": a["x2"], "cand_cost": a["cand"], "cg_it": a["it"], "cg_broke": a["done"] == 2,
             "force_invalid": bool(a["dbg"])} for a in s["attempts"]]


def device_run(ctx, s, plan=(), **kw):
    a = s["attempts"]
    arrays = {"xbr": [x["xbr"] for x in a], "d2xx": [x["d2xx"] for x in a], "pcg_it": [x["it"] for x in a], "pcg_done": [x["done"] for x in a],
              "norms2": [[x["step2"], x["x2"]] for x in a], "cand_cost": [x["cand"] for x in a], "debug_invalid": [x["dbg"] for x in a]}
    return ctx.debug_lm_script(s["cost"], s["ngrad"], s["nfree"], s["radius0"], s["lm_steps"], arrays, plan=plan, **kw)


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def ulps64(a, b):
    """distance in units of the last place between two finite fp64 of the same sign"""
    return abs(int(bits(a)) - int(bits(b)))


_seen = {"ulp": 0, "scripts": 0, "resyncs": {p: 0 for p in PLANS}}
INT_FIELDS = ("final_", "accepted", "pcg_it", "termination", "kind")
F64_FIELDS = ("cost", "cand_cost", "model_change", "rel", "radius_after")


def compare_with_twin(dev, twin, name):
    assert len(dev) == len(twin), (name, len(dev), len(twin), [int(k) for k in dev["kind"]], [r["kind"] for r in twin])
    for i, (d, t) in enumerate(zip(dev, twin)):
        for f in INT_FIELDS:
            assert int(d[f]) == t[f], (name, i, f, int(d[f]), t[f], t["what"])
        for f in F64_FIELDS:
            if f == "radius_after" and t["accepted"]:
                u = ulps64(d[f], t[f]); _seen["ulp"] = max(_seen["ulp"], u)
                assert u <= 8, (name, i, "radius after an accepted step", float(d[f]), t[f], u)
            else:                  # (a NaN is a NaN: its payload is not part of the statement)
                assert bits(d[f]) == bits(t[f]) or (np.isnan(d[f]) and np.isnan(t[f])), (name, i, f, float(d[f]), t[f], t["what"])


def check_ran(res, i, K=0):
    """setup i was written by a begin kernel: no NaN inside, the guards intact"""
    NB, NS = 36 * K + 41, 6 * K + 9
    b, d = res["blocks"][i], res["d2"][i]
    assert not np.isnan(b[G:G + NB]).any() and not np.isnan(d[G:G + NS]).any()
    assert np.isnan(b[:G]).all() and np.isnan(b[G + NB:]).all() and np.isnan(d[:G]).all() and np.isnan(d[G + NS:]).all()


@pytest.mark.parametrize("s", SCRIPTS, ids=[s["name"] for s in SCRIPTS])
def test_script_against_the_twin_and_the_ladder_against_the_serial_loop(ctx, s):
    _seen["scripts"] += 1
    # the twin alone: the named branch is reached
    trecs, tst, tradii = T.run_script(s["cost"], s["ngrad"], s["nfree"], s["radius0"], s["lm_steps"], twin_inputs(s))
    ok = s["expect"](trecs) if callable(s["expect"]) else trecs[-1]["what"] == s["expect"]
    assert ok, (s["name"], whats(trecs))
    # the serial loop of the device against the twin
    ser = device_run(ctx, s)
    compare_with_twin(ser["records"], trecs, s["name"])
    st = ser["state"]
    assert (st["done"], st["termination"], st["invalid"], st["attempts"], st["successful"]) == (1, tst["termination"], tst["invalid"], tst["attempts"], tst["successful"]), (st, tst)
    assert bits(st["cost"]) == bits(tst["cost"]) and bits(st["decrease_factor"]) == bits(tst["nu"])
    assert bits(st["radius"]) == bits(tst["radius"]) or (tst["successful"] and ulps64(st["radius"], tst["radius"]) <= 8)
    begun = [i for i in range(len(ser["meta"])) if not np.isnan(ser["blocks"][i][G])]
    assert len(begun) == len(tradii)
    serial_radius = {}
    for i, r in zip(begun, tradii):
        check_ran(ser, i)
        assert int(ser["meta"][i][0]) == i and bits(ser["radius"][i]) == bits(r) and ser["inv_radius"][i] == np.float32(1.0 / r), (s["name"], i, ser["radius"][i], r)
        serial_radius[i] = ser["radius"][i]
    # every batch plan against the serial loop and against the twin's statement of the ladder
    for plan in PLANS:
        lrecs, lst, resyncs, setups = T.run_script_ladder(s["cost"], s["ngrad"], s["nfree"], s["radius0"], s["lm_steps"], twin_inputs(s), plan)
        lad = device_run(ctx, s, plan=plan)
        R = lad["records"]
        assert [int(k) for k in R["kind"]] == [r["kind"] for r in lrecs], (s["name"], plan, [int(k) for k in R["kind"]], [r["kind"] for r in lrecs])
        assert int((R["kind"] == 3).sum()) == resyncs, (s["name"], plan)
        _seen["resyncs"][plan] += resyncs
        kept = R[R["kind"] != 3]
        assert len(kept) == len(ser["records"])
        for f in INT_FIELDS + F64_FIELDS + ("ngrad", "nfree"):
            assert np.array_equal(kept[f].view(np.int32 if f in INT_FIELDS else np.int64), ser["records"][f].view(np.int32 if f in INT_FIELDS else np.int64)), (s["name"], plan, f)
        for r3, t3 in zip(R[R["kind"] == 3], [r for r in lrecs if r["kind"] == 3]):
            assert (int(r3["final_"]), int(r3["accepted"]), int(r3["pcg_it"])) == (0, 0, 0) and bits(r3["radius_after"]) == bits(t3["radius_after"]) and bits(r3["cost"]) == bits(t3["cost"])
        for f in ("cost", "radius", "decrease_factor", "termination", "invalid", "attempts", "successful"):
            assert bits(lad["state"][f]) == bits(ser["state"][f]), (s["name"], plan, f)
        assert lad["state"]["done"] == 1
        # the set-up of every batch: the radii of j rejections in a row, dead systems untouched
        flat = [x for batch in setups for x in batch]
        assert len(flat) == len(lad["meta"]), (s["name"], plan, len(flat), len(lad["meta"]))
        last = {}
        for i, (attempt, radius) in enumerate(flat):
            m = lad["meta"][i]
            if radius is None:          # the batch whose first attempt found the radius run out: nothing is set up
                assert int(m[0]) == attempt and np.isnan(lad["blocks"][i]).all() and np.isnan(lad["d2"][i]).all(), (s["name"], plan, i)
                continue
            assert int(m[0]) == attempt and bits(lad["radius"][i]) == bits(radius), (s["name"], plan, i, m, lad["radius"][i], radius)
            if radius < 1e-32:
                assert lad["inv_radius"][i] == 0.0 and np.isnan(lad["blocks"][i]).all() and np.isnan(lad["d2"][i]).all(), (s["name"], plan, i)
            else:
                assert lad["inv_radius"][i] == np.float32(1.0 / radius)
                check_ran(lad, i)
            assert np.isnan(lad["minv"][i]).all()          # the ladder's 1x1 inverses are recomputed by its vector kernels
            last[attempt] = lad["radius"][i]
        # a decided attempt was solved at the radius the serial loop holds there
        for a in range(int(ser["state"]["attempts"])):
            assert bits(last[a]) == bits(serial_radius[a]), (s["name"], plan, a, last[a], serial_radius[a])


def test_invalid_first_attempt_is_out_of_step_one_rejection_later(ctx):
    """decrease_factor is still 2 at the first attempt: radius * 0.5 and radius / 2 are the same bits, so a batch is NOT out of step behind an invalid first attempt.
    One rejection later 2500 != 1250, and attempt 2 is solved again alone."""
    s = next(x for x in SCRIPTS if x["name"] == "invalid at 0 by flag")
    for plan, want in (((6,), [0, 1, 1, 3, 1, 1]), ((2,), [0, 1, 1, 1, 1]), ((4,), [0, 1, 1, 3, 1, 1])):
        lad = device_run(ctx, s, plan=plan)
        assert [int(k) for k in lad["records"]["kind"]] == want, (plan, lad["records"]["kind"])
        if 3 in want:
            r3 = lad["records"][3]
            assert float(r3["radius_after"]) == 2500.0 and float(lad["radius"][2]) == 1250.0 and float(lad["radius"][1]) == 5000.0
            assert float(lad["radius"][plan[0]]) == 2500.0 and int(lad["meta"][plan[0]][2]) == 1      # the batch of one that follows
    s1 = next(x for x in SCRIPTS if x["name"] == "invalid at 1")
    lad = device_run(ctx, s1, plan=(6,))
    assert [int(k) for k in lad["records"]["kind"]] == [0, 1, 1, 3, 1, 1, 1]


# ---------------------------------------------------------------- the block-Jacobi setup ----------------------------------------------------------------

def make_blocks(K, seed):
    """camera blocks of J^T J: pose blocks 6x6, intrinsics 4x4, distortion 5x5.  Regular blocks: a correlation matrix of condition <= 1e3 scaled by column norms within
    a factor 10 of a block magnitude that spans 1e-9 .. 1e17 over the blocks (squared norms up to 1e35).  Special blocks: one indefinite, one with a zero column."""
    rng = np.random.default_rng(seed)
    sizes = [6] * K + [4, 5]
    nblk = len(sizes)
    special = {"zero": nblk - 2 if K < 3 else 1, "indef": nblk - 1 if K < 3 else 2}
    mags = 10.0 ** rng.uniform(-9.0, 16.5, nblk); mags[0] = 1e-9; mags[-1] = 10.0 ** 16.5
    if K >= 1:
        mags[K - 1] = 3e16                                            # the last pose block, and the two blocks behind it: the tail of a 64-thread workgroup at K = 63 .. 65
    cd, tr, kinds = [], [], []
    for b, n in enumerate(sizes):
        A = rng.standard_normal((n + 3, n)); C = A.T @ A + 0.05 * np.eye(n) * n
        d = 1.0 / np.sqrt(np.diag(C)); C = C * np.outer(d, d)         # unit diagonal
        assert np.linalg.cond(C) <= 1e3
        norms = mags[b] * 10.0 ** rng.uniform(0.0, 1.0, n)
        H = C * np.outer(norms, norms); kind = "regular"
        if b == special["indef"]:
            H[0, 1] = H[1, 0] = 3.0 * np.sqrt(H[0, 0] * H[1, 1]); kind = "indef"
        if b == special["zero"]:
            H[2, :] = 0.0; H[:, 2] = 0.0; kind = "zero"
        cd.append(np.diag(H).copy()); tr.append(H[np.triu_indices(n)]); kinds.append(kind)
    return sizes, np.concatenate(cd), np.concatenate(tr), kinds


def make_tail(cdiag, seed):
    """the camera tail as the vector kernels hold it (float32 squared norms, Jacobi scaling).  A few entries carry a scaling that does not belong to their norm, so that
    c S^2 exceeds 1e32 and falls below 1e-6: both clamps; a few are fixed (S = 0)."""
    rng = np.random.default_rng(seed)
    c = cdiag.astype(np.float32)
    S = (np.float32(1) / (np.float32(1) + np.sqrt(c))).astype(np.float32)
    n = c.size
    S[rng.choice(n, max(2, n // 7), replace=False)] = 0.0
    hi = rng.choice(n, 3, replace=False); c[hi] = np.float32(1e35); S[hi] = 1.0
    return c, S


def split(sizes, flat, sq):
    out, o = [], 0
    for n in sizes:
        m = n * n if sq else n
        out.append(flat[o:o + m]); o += m
    return out


def ulps32(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64); b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


_blk = {"worst": 0.0, "kappa": 0.0}


def check_setup(res, i, K, sizes, cdiag, tri, kinds, fix, radius, tc, tS, serial):
    NB, NS = 36 * K + 41, 6 * K + 9
    check_ran(res, i, K)
    blocks = res["blocks"][i][G:G + NB]
    # device layout: pose block k at 36 k, intrinsics at 36 K, distortion at 36 K + 16
    offs = [36 * k for k in range(K)] + [36 * K, 36 * K + 16]
    cds = split(sizes, cdiag, False); o = 0
    for b, n in enumerate(sizes):
        t = tri[o:o + n * (n + 1) // 2]; o += n * (n + 1) // 2
        fixed = fix[0] if b < K else fix[1] if b == K else fix[2]
        ref, kappa, fell_back = T.cam_blocks(cds[b], t, fixed, radius)
        dev = blocks[offs[b]:offs[b] + n * n].reshape(n, n).astype(np.float64)
        if fixed:
            assert np.all(dev == 0.0), (K, b)
            continue
        big = np.abs(ref).max()
        bound = float(np.spacing(np.float32(big))) + 64.0 * kappa * 2.0 ** -52 * big
        err = np.abs(dev - ref.astype(np.float32).astype(np.float64)).max()
        _blk["worst"] = max(_blk["worst"], err / bound); _blk["kappa"] = max(_blk["kappa"], kappa)
        assert err <= bound, (K, b, kinds[b], radius, err, bound, kappa)
        if kinds[b] == "regular":
            assert kappa <= 1e6 and not fell_back
        if fell_back:
            assert np.count_nonzero(dev - np.diag(np.diag(dev))) == 0
    d2_ref, minv_ref = T.tail_diag(tc, tS, np.float32(1.0 / radius))
    d2 = res["d2"][i][G:G + NS]
    assert np.array_equal(d2.view(np.int32), d2_ref.view(np.int32)), (K, radius, np.flatnonzero(d2.view(np.int32) != d2_ref.view(np.int32))[:5])
    assert np.all(d2[tS == 0] == 0)
    if serial:
        minv = res["minv"][i]
        assert np.isnan(minv[:G]).all() and np.isnan(minv[G + NS:]).all()
        minv = minv[G:G + NS]
        same = minv == minv_ref
        assert np.all(same | (ulps32(minv, minv_ref) <= 2)), (K, radius, minv[~same][:5], minv_ref[~same][:5])
        assert np.all(minv[tS == 0] == 0)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
def test_block_jacobi_setup_against_numpy_and_the_ladder_against_the_serial_loop(ctx, K):
    sizes, cdiag, tri, kinds = make_blocks(K, seed=100 + K)
    assert set(kinds) == {"regular", "indef", "zero"}
    tc, tS = make_tail(cdiag, seed=200 + K)
    one = script("one attempt", [rej()], "reject+limit")
    for radius in (1e4, 1.0, 1e-20):
        for fix in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            if fix != (0, 0, 0) and radius != 1.0:
                continue
            one["radius0"] = radius
            res = device_run(ctx, one, K=K, fix=fix, cdiag=cdiag, tri=tri, tail_c=tc, tail_S=tS)
            assert bits(res["radius"][0]) == bits(radius)
            check_setup(res, 0, K, sizes, cdiag, tri, kinds, fix, radius, tc, tS, serial=True)
    # a batch of six from radius 1: system j against numpy and, bit for bit, against the serial loop's k_lm_begin started at that radius
    six = script("six rejected", [rej()] * 6, "reject+limit", radius0=1.0)
    lad = device_run(ctx, six, plan=(6,), K=K, cdiag=cdiag, tri=tri, tail_c=tc, tail_S=tS)
    radii = T.ladder_radii(1.0, 2.0, 6)
    assert len(lad["meta"]) == 6
    for j, radius in enumerate(radii):
        assert bits(lad["radius"][j]) == bits(radius)
        check_setup(lad, j, K, sizes, cdiag, tri, kinds, (0, 0, 0), radius, tc, tS, serial=False)
        one["radius0"] = radius
        ser = device_run(ctx, one, K=K, cdiag=cdiag, tri=tri, tail_c=tc, tail_S=tS)
        assert np.array_equal(ser["blocks"][0].view(np.int32), lad["blocks"][j].view(np.int32)), (K, j)
        assert np.array_equal(ser["d2"][0].view(np.int32), lad["d2"][j].view(np.int32)), (K, j)


def test_report():
    """what the module measured (run with -s to read it)"""
    print(f"\n[lm controller] largest ulp distance of an accepted radius from the twin: {_seen['ulp']} (bound 8)")
    print(f"[lm controller] largest block-inverse error / bound: {_blk['worst']:.3g} (largest condition number {_blk['kappa']:.3g})")
    print("[lm controller] kind-3 records (resyncs) over all scripts, per batch plan: " + ", ".join(f"{list(p)}: {n}" for p, n in _seen["resyncs"].items()))
    assert _seen["ulp"] <= 8 and _blk["worst"] <= 1.0
    assert _seen["scripts"] < len(SCRIPTS) or all(n > 0 for n in _seen["resyncs"].values())
