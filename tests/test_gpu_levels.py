"""-m gpu: level transitions, recolourisation and the refine schedule through the C ABI, against the oracle.

Everything that is index / byte work is held to bit-exactness INCLUDING the visit order of the voxels (the reference's results
depend on its unordered_map iteration order): loaded .tsdf records -> converted grid, thin-shell sparsification, x2 upsampling,
8-bit recolourisation.  The multi-level refine is held to the north-star tolerance on SDF / albedo."""
import numpy as np
import pytest

import helpers
from bench_slice import color_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(oracle):
    sc = helpers.small_scene(seed=5, radius_vox=12, K=7, width=128, height=96, levels=2)
    sc = dict(sc); sc["frames"] = color_frames(sc)
    return sc


def _same_grid(a, b, exact_fields=("keys", "weight", "color", "sdf", "sdf_refined", "albedo")):
    assert a["keys"].shape == b["keys"].shape
    for k in exact_fields:
        assert np.array_equal(a[k], b[k]), k


def test_tsdf_records_to_visit_order(oracle, scene):
    from intrinsic3d_amd import binding
    sc = scene
    rng = np.random.default_rng(0)
    keys = sc["keys"].copy(); sdf = sc["sdf"].copy(); w = sc["weight"].copy(); col = sc["color"].copy()
    w[rng.integers(0, len(w), 50)] = 0.0                       # invalid records are dropped by convert()
    keys = np.concatenate([keys, keys[:5]]); sdf = np.concatenate([sdf, sdf[:5] + 0.001]).astype(np.float32)   # duplicate keys: last record wins
    w = np.concatenate([w, np.ones(5, np.float32)]); col = np.concatenate([col, col[:5]])
    g = oracle.Grid.from_voxels(sc["voxel_size"], keys, sdf, w, col)
    with binding.Context(0) as ctx:
        ctx.set_grid_from_tsdf_records(sc["voxel_size"], keys, sdf, w, col)
        out = ctx.export_grid()
        n, vs, tr = ctx.grid_info()
    ref = g.export()
    assert n == len(g) and vs == float(np.float32(sc["voxel_size"]))
    _same_grid(out, ref)
    g.free()


def test_recompute_colors_bit_exact(oracle, scene):
    from intrinsic3d_amd import binding
    sc = scene
    for nobs in (5, 0, 2):
        g = oracle.Grid.from_voxels(sc["voxel_size"], sc["keys"], sc["sdf"], sc["weight"], sc["color"])
        fr = oracle.Frames(sc["frames"], sc["levels"])
        a = g.export()
        with binding.Context(0) as ctx:
            ctx.set_grid(sc["voxel_size"], a["keys"], a["sdf"], a["sdf_refined"], a["albedo"], a["weight"], a["color"])
            ctx.set_frames(sc["frames"], sc["levels"]); ctx.set_camera(sc["intr"], sc["dist"], sc["poses"])
            ctx.recompute_colors(0.02, nobs)
            out = ctx.export_grid()
        oracle.recompute_colors(g, fr, sc["intr"], sc["dist"], sc["poses"], 0.02, nobs)
        ref = g.export()
        changed = np.any(ref["color"] != a["color"], axis=1).sum()
        assert changed > 0.2 * len(g)                            # the test must exercise the recolouring
        diff = np.abs(out["color"].astype(int) - ref["color"].astype(int))
        assert diff.max() == 0, (nobs, int((diff > 0).sum()), int(diff.max()))
        g.free(); fr.free()


def test_thin_shell_and_upsample_bit_exact(oracle, scene):
    from intrinsic3d_amd import binding
    sc = scene
    g = oracle.Grid.from_voxels(sc["voxel_size"], sc["keys"], sc["sdf"], sc["weight"], sc["color"])
    a = g.export()
    rng = np.random.default_rng(2)                               # distinct sdf_refined / albedo so every field is exercised
    sr = a["sdf_refined"] + rng.normal(0, 0.05 * float(sc["voxel_size"]), len(g)); al = 0.6 + rng.normal(0, 0.05, len(g))
    g.import_fields(sdf_refined=sr, albedo=al)
    a = g.export()
    thres = 1.0 * float(sc["voxel_size"])
    with binding.Context(0) as ctx:
        ctx.set_grid(sc["voxel_size"], a["keys"], a["sdf"], a["sdf_refined"], a["albedo"], a["weight"], a["color"])
        n1 = ctx.clear_outside_thin_shell(thres)
        g.clear_outside_shell(thres)
        assert n1 == len(g) and n1 < len(a["weight"])
        _same_grid(ctx.export_grid(), g.export())
        # level transition: 8 children per voxel, new map order, halved voxel size
        n2 = ctx.upsample()
        up = g.upsample()
        assert n2 == len(up) == 8 * n1
        out, ref = ctx.export_grid(), up.export()
        _same_grid(out, ref)
        assert (ref["weight"] <= 0).any() and (ref["weight"] > 0).any()
        n, vs, tr = ctx.grid_info()
        assert vs == up.voxel_size and tr == float(np.float32(vs) * np.float32(5.0))
        # and once more on the fine grid (invalid voxels present now)
        thres2 = 1.5 * vs
        n3 = ctx.clear_outside_thin_shell(thres2); up.clear_outside_shell(thres2)
        assert n3 == len(up)
        _same_grid(ctx.export_grid(), up.export())
        up.free()
    g.free()


def _oracle_refine(oracle, sc, ocfg, pose_eps=0.0):
    g = oracle.Grid.from_voxels(sc["voxel_size"], sc["keys"], sc["sdf"], sc["weight"], sc["color"])
    fr = oracle.Frames(sc["frames"], sc["levels"])
    poses0 = np.array(sc["poses"], np.float64) * (1.0 + pose_eps)
    rcode, intr, dist, poses, done = oracle.refine(g, fr, ocfg, 2, 2, 2.0, 1.0, 1, 0.05, 10.0, sc["intr"], sc["dist"], poses0)
    assert rcode == 0 and done == 3
    ref = g.export(); g.free(); fr.free()
    return ref, intr, poses


@pytest.mark.parametrize("iterations,fix_intrinsics", [(1, 0), (2, 1)])
def test_refine_two_levels_matches_oracle(oracle, scene, iterations, fix_intrinsics):
    """Intrinsic3D::refine: 2 grid levels x 2 pyramid levels = 3 lighting + optimize + recolour rounds, one sparsification per level,
    one upsampling.  Structure (keys, order, validity) must be identical up to the handful of voxels that sit within round-off of a thin-shell
    threshold (helpers.align_by_key).  Fields are held to 1e-4 relative — or, where the joint
    geometry + pose problem is so ill-conditioned (gauge freedom) that the ORACLE ITSELF moves further than that when its input poses
    are perturbed by a few 1e-7 relative, to helpers.ENVELOPE_FACTOR x that measured sensitivity envelope (five perturbed re-runs) of the reference
    computation."""
    from intrinsic3d_amd import binding
    sc = scene
    ocfg = helpers.oracle_cfg(oracle, 0.0, iterations=iterations, lm_steps=20, fix_distortion=1, fix_intrinsics=fix_intrinsics)
    seen = []
    with binding.Context(0) as ctx:
        ctx.set_grid_from_tsdf_records(sc["voxel_size"], sc["keys"], sc["sdf"], sc["weight"], sc["color"])
        ctx.set_frames(sc["frames"], sc["levels"]); ctx.set_camera(sc["intr"], sc["dist"], sc["poses"])
        rc = binding.RefineConfig(num_grid_levels=2, num_rgbd_levels=2, thin_shell_factor=2.0, thin_shell_factor_final=1.0, clear_distant_voxels=1,
                                  occlusion_distance=0.02, num_observations=5, subvolume_size_sh=0.05, sh_lambda_reg=10.0)
        ctx.refine(rc, helpers.gpu_cfg(ocfg), callback=lambda gl, ng, pl, npl: seen.append((gl, pl, ctx.grid_info()[0])))
        out = ctx.export_grid(); intr, dist, poses = ctx.get_camera()
    assert [(a, b) for a, b, _ in seen] == [(1, 1), (1, 0), (0, 0)]          # all pyramid levels only on the coarsest grid
    ref, ointr, oposes = _oracle_refine(oracle, sc, ocfg)
    ref_full = ref
    out, ref = helpers.align_by_key(out, ref)                                 # (a voxel within round-off of a thin-shell threshold may be kept on one side only)
    assert (out["weight"] != ref["weight"]).mean() <= 2e-4
    # conditioning envelope of the reference computation: the oracle re-run with its input poses perturbed by a few 1e-7 (relative)
    env = dict(sdf_refined=0.0, albedo=0.0, intr=0.0, poses=0.0)
    for eps in (1e-7, -1e-7, 3e-7, -3e-7, 1e-6):
        per, pintr, pposes = _oracle_refine(oracle, sc, ocfg, pose_eps=eps)
        if per["keys"].shape == ref_full["keys"].shape and np.array_equal(per["keys"], ref_full["keys"]):
            for k in ("sdf_refined", "albedo"):
                env[k] = max(env[k], float(np.abs(per[k] - ref_full[k]).max()))
        env["intr"] = max(env["intr"], float(np.abs(pintr - ointr).max())); env["poses"] = max(env["poses"], float(np.abs(pposes - oposes).max()))
    d_sdf = np.abs(out["sdf_refined"] - ref["sdf_refined"]); d_alb = np.abs(out["albedo"] - ref["albedo"])
    smax = float(np.abs(ref["sdf_refined"]).max())
    assert np.median(d_sdf) <= 1e-5 * smax and np.median(d_alb) <= 1e-5
    assert np.quantile(d_sdf, 0.999) <= max(1e-4 * smax, env["sdf_refined"]) and np.quantile(d_alb, 0.999) <= max(1e-4, env["albedo"])
    # isolated voxels next to a marginal decision (row validity, observation choice) may move further, in the oracle's own perturbed runs too
    print("two-level refine: max |d sdf| / smax", d_sdf.max() / smax, "max |d albedo|", d_alb.max(), "envelope", env, "smax", smax)
    assert d_sdf.max() <= max(1e-4 * smax, helpers.ENVELOPE_FACTOR * env["sdf_refined"]), (d_sdf.max(), smax, env)
    assert d_alb.max() <= max(1e-4, helpers.ENVELOPE_FACTOR * env["albedo"]), (d_alb.max(), env)
    assert np.abs(intr - ointr).max() <= max(1e-5 * np.abs(ointr).max(), helpers.ENVELOPE_FACTOR * env["intr"])
    assert np.abs(poses - oposes).max() <= max(1e-5, helpers.ENVELOPE_FACTOR * env["poses"]), (np.abs(poses - oposes).max(), env)
    cd = np.abs(out["color"].astype(int) - ref["color"].astype(int))
    assert (cd > 1).mean() < 1e-3                                             # 8-bit truncation of colours computed from ~1e-7-different geometry


def test_keyframe_pyramids_on_device_bit_exact(oracle):
    """Pyramid::create on the device (i3d_set_frames_rgbd): luminance from 8-bit BGR, pyrDown levels, valid-mean depth levels == oracle, bit for bit"""
    from intrinsic3d_amd import binding
    rng = np.random.default_rng(4)
    K, W, H, L = 3, 101, 75, 3                     # odd sizes: the (w/2, h/2) floor and the reflected borders are exercised
    bgr = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(K)]
    dep = []
    for _ in range(K):
        d = rng.uniform(0.4, 3.0, (H, W)).astype(np.float32); d[rng.uniform(size=d.shape) < 0.25] = 0.0; dep.append(d)
    with binding.Context(0) as ctx:
        ctx.set_frames_rgbd(bgr, dep, L)
        for f in range(K):
            lum_ref = oracle.lum_from_bgr(bgr[f]); dep_ref = dep[f]; w, h = W, H
            for l in range(L):
                lum, d = ctx.get_frame_image(f, l, w, h)
                assert np.array_equal(lum, lum_ref), (f, l, np.abs(lum - lum_ref).max())
                assert np.array_equal(d, dep_ref), (f, l)
                lum_ref = oracle.pyr_down(lum_ref); dep_ref = oracle.depth_down(dep_ref); w //= 2; h //= 2


def test_refine_sharded_ranks_match_single_rank(oracle, scene):
    """the whole refine schedule under the SPMD path (2 ranks simulated by 2 host threads on one GPU): level transitions, lighting and
    recolourisation run replicated, the optimisation sharded; every rank must end with the single-rank grid"""
    import threading
    from intrinsic3d_amd import binding
    sc = scene
    # intrinsics fixed: with them free this tiny scene is so ill-conditioned that two runs of the SAME single-rank binary (fp32 atomics ->
    # run-to-run summation order) already differ by ~1e-4 in albedo after the three optimisations of the schedule
    ocfg = helpers.oracle_cfg(oracle, 0.0, iterations=1, lm_steps=20, fix_distortion=1, fix_intrinsics=1, cg_fixed_iterations=8)
    rc = binding.RefineConfig(num_grid_levels=2, num_rgbd_levels=2, thin_shell_factor=2.0, thin_shell_factor_final=1.0, clear_distant_voxels=1,
                              occlusion_distance=0.02, num_observations=5, subvolume_size_sh=0.05, sh_lambda_reg=10.0)

    def make():
        c = binding.Context(0)
        c.set_grid_from_tsdf_records(sc["voxel_size"], sc["keys"], sc["sdf"], sc["weight"], sc["color"])
        c.set_frames(sc["frames"], sc["levels"]); c.set_camera(sc["intr"], sc["dist"], sc["poses"])
        return c
    ref = make(); ref.refine(rc, helpers.gpu_cfg(ocfg)); want = ref.export_grid(); wcam = ref.get_camera(); ref.close()
    L = binding.load(); W = 2
    shared = L.i3d_comm_sim_create(W)
    ctxs = [make() for _ in range(W)]
    for r, c in enumerate(ctxs):
        c.comm_init_sim(shared, r)
    err = [None] * W

    def run(r):
        try:
            ctxs[r].refine(rc, helpers.gpu_cfg(ocfg))
        except Exception as e:
            err[r] = e
    th = [threading.Thread(target=run, args=(r,)) for r in range(W)]
    [t.start() for t in th]; [t.join(timeout=300) for t in th]
    assert not any(t.is_alive() for t in th), "sharded refine hung"
    assert all(e is None for e in err), err
    for c in ctxs:
        got = c.export_grid(); cam = c.get_camera()
        assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["weight"], want["weight"])
        smax = np.abs(want["sdf_refined"]).max()
        assert np.abs(got["sdf_refined"] - want["sdf_refined"]).max() <= 1e-4 * smax
        assert np.abs(got["albedo"] - want["albedo"]).max() <= 3e-4
        assert np.array_equal(cam[0], wcam[0]); np.testing.assert_allclose(cam[2], wcam[2], rtol=1e-3, atol=1e-5)
        c.close()
    L.i3d_comm_sim_destroy(shared)


def test_resize_depth_bit_exact(oracle):
    """resizeDepth: a 320x240 depth image (holes, zero border) into a 640x480 colour camera with different intrinsics, and a 2x down case"""
    from intrinsic3d_amd import binding
    rng = np.random.default_rng(6)
    d = rng.uniform(0.5, 3.0, (240, 320)).astype(np.float32); d[rng.uniform(size=d.shape) < 0.2] = 0.0
    for (ow, oh, oi) in ((640, 480, [525.0, 524.0, 319.5, 239.5]), (160, 120, [131.0, 131.5, 80.2, 59.1]), (700, 500, [400.0, 400.0, 350.0, 250.0])):
        ii = [262.5, 262.0, 159.5, 119.5]
        got = binding.resize_depth(d, ii, ow, oh, oi); ref = oracle.resize_depth(d, ii, ow, oh, oi)
        assert (ref > 0).mean() > 0.3 and np.array_equal(got, ref), (ow, oh, np.abs(got - ref).max())
    assert np.array_equal(binding.resize_depth(d, ii, 320, 240, oi), d)          # same size: clone


def test_device_level_operations_match_committed_golden():
    """the device path alone against tests/golden/levels_small.json (CRCs of byte-exact stages of the ORACLE's convert / recolour / thin-shell / upsample /
    resizeDepth / pyramid restatements on seeded inputs, tests/golden/make_golden.py — regression vectors, not reference outputs): needs no oracle library at run time"""
    import json, os, zlib
    from intrinsic3d_amd import binding
    import golden.make_golden as mg
    gold = mg.strip_tags(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels_small.json"))))
    crc = lambda a: int(zlib.crc32(np.ascontiguousarray(a).tobytes()))
    sc = mg.level_scene()
    with binding.Context(0) as ctx:
        ctx.set_grid_from_tsdf_records(sc["voxel_size"], sc["keys"], sc["sdf"], sc["weight"], sc["color"])
        ctx.set_frames(sc["frames"], 1); ctx.set_camera(sc["intr"], sc["dist"], sc["poses"])
        a = ctx.export_grid()
        assert {"n": len(a["weight"]), "keys": crc(a["keys"])} == gold["convert"]
        ctx.recompute_colors(0.02, 3)
        assert crc(ctx.export_grid()["color"]) == gold["recolor"]["color"]
        n = ctx.clear_outside_thin_shell(1.5 * float(sc["voxel_size"]))
        assert {"n": n, "keys": crc(ctx.export_grid()["keys"])} == gold["thin_shell"]
        n = ctx.upsample(); b = ctx.export_grid()
        got = {"n": n, "keys": crc(b["keys"]), "weight": crc(b["weight"]), "sdf": crc(b["sdf"]), "color": crc(b["color"]), "valid": int((b["weight"] > 0).sum())}
        assert got == gold["upsample"]
        bgr = sc["frames"][0]["bgr"][0]; dep = sc["frames"][0]["depth"][0]; h, w = dep.shape
        ctx.set_frames_rgbd([bgr], [dep], 3)
        l0, _ = ctx.get_frame_image(0, 0, w, h); l1, d1 = ctx.get_frame_image(0, 1, w // 2, h // 2); l2, _ = ctx.get_frame_image(0, 2, w // 4, h // 4)
        assert {"lum0": crc(l0), "lum1": crc(l1), "lum2": crc(l2), "depth1": crc(d1)} == gold["pyramid"]
    assert crc(binding.resize_depth(dep, [78.75, 78.0, 47.5, 35.5], 160, 120, [131.0, 131.5, 80.2, 59.1])) == gold["resize_depth"]["crc"]


def test_map_order_on_the_device_matches_the_standard_container():
    """device/map_order.hip (one atomicMin + radix sort per rehash epoch) against a real std::unordered_map with the reference's hash,
    reserve(64) and load factor 0.6: sizes around the first rehash points, a size with ~14 epochs, negative coordinates."""
    from intrinsic3d_amd import binding as B
    rng = np.random.default_rng(4)
    grid = np.stack(np.meshgrid(np.arange(-50, 50), np.arange(-45, 55), np.arange(-3, 77), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    rng.shuffle(grid)
    for n in [1, 2, 39, 40, 41, 42, 63, 64, 65, 100, 1000, 4096, 65537, 300000, len(grid)]:
        k = grid[:n]
        got = B.debug_map_order(k, 4)
        assert len(got) == n and np.array_equal(got, B.debug_map_order(k, 2)), n


def test_every_order_crossing_round_trips_bit_for_bit():
    """device order <-> the caller's order, once through every crossing, on the smallest grid at which one can go wrong: a 10 x 7 x 5 box of 350 voxels with
    its corner at (-5, -3, -2) (more than one 8^3 brick, negative coordinates, two 256-thread workgroups with a ragged tail), its keys handed over in a seeded
    shuffle so that the device permutation is not the identity.  Every field holds values that name their voxel.  No oracle: the expected values are the inputs."""
    from intrinsic3d_amd import binding
    rng = np.random.default_rng(11)
    keys = (np.stack(np.meshgrid(np.arange(10), np.arange(7), np.arange(5), indexing="ij"), -1).reshape(-1, 3) + [-5, -3, -2]).astype(np.int32)
    keys = keys[rng.permutation(len(keys))]
    n = len(keys); assert n == 350
    vs = 0.01
    sent = dict(keys=keys, sdf=rng.normal(0, vs, n), sdf_refined=rng.normal(0, vs, n), albedo=rng.uniform(0.1, 0.9, n),
                weight=rng.uniform(0.5, 2.0, n).astype(np.float32), color=rng.integers(0, 256, (n, 3)).astype(np.uint8))
    with binding.Context(0) as ctx:
        ctx.set_grid(vs, *[sent[k] for k in ("keys", "sdf", "sdf_refined", "albedo", "weight", "color")])
        _same_grid(ctx.export_grid(), sent)                                       # set_grid -> export_grid
        # debug_neighbors: a dictionary look-up of the keys, all 18 offsets (common.hpp nbr_offset)
        index = {tuple(k): i for i, k in enumerate(keys.tolist())}
        offs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1),
                (-2, 0, 0), (0, -2, 0), (0, 0, -2), (-1, -1, 0), (-1, 0, -1), (0, -1, -1)]
        want_nb = np.array([[index.get((k[0] + o[0], k[1] + o[1], k[2] + o[2]), -1) for o in offs] for k in keys.tolist()], np.int32)
        nb = ctx.debug_neighbors()
        assert np.array_equal(nb, want_nb) and (want_nb >= 0).all(axis=1).any() and (want_nb < 0).any()
        # update_grid -> get_grid / export_grid
        # (the new surface is the plane x = -0.5, jittered so that every value still names its voxel: the shell below then keeps x in -2 .. 2, half of the box)
        upd = dict(sdf_refined=(keys[:, 0] + 0.5 + rng.uniform(-0.1, 0.1, n)) * vs, albedo=rng.uniform(0.1, 0.9, n), color=rng.integers(0, 256, (n, 3)).astype(np.uint8))
        ctx.update_grid(**upd)
        sr, al = ctx.get_grid()
        assert np.array_equal(sr, upd["sdf_refined"]) and np.array_equal(al, upd["albedo"])
        _same_grid(ctx.export_grid(), dict(sent, **upd))
        # set_voxel_sh -> get_voxel_sh: stored as float32
        sh = rng.normal(0, 1, (n, 9))
        ctx.set_voxel_sh(sh)
        assert np.array_equal(ctx.get_voxel_sh(), sh.astype(np.float32).astype(np.float64))
        # clear_outside_thin_shell keeps the survivors in the caller's relative order, each with all of its record
        before = ctx.export_grid()
        m = ctx.clear_outside_thin_shell(vs)
        after = ctx.export_grid()
        assert 0 < m < n and len(after["weight"]) == m
        where = np.array([index[tuple(k)] for k in after["keys"].tolist()])
        assert np.all(np.diff(where) > 0)                                          # a stable filter of the caller's order
        _same_grid(after, {k: v[where] for k, v in before.items()})
        assert sorted(set(after["keys"][:, 0].tolist())) == [-2, -1, 0, 1, 2] and m == 5 * 35
