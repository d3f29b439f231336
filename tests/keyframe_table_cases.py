"""Scenes whose waves meet more keyframes than a per-wave keyframe table holds (shared by tests/test_oracle_cpu.py and tests/test_gpu_edge_cases.py; not collected).

Every kernel that sums the pose columns of the Eg rows goes through a table private to the wave (wave_ops.hpp: wave_table_add / wave_table_add_quads,
tile_pass_mr.hip: mr_table_add): 32 slots in k_eg_tile_mr, k_eg_tile<512> and the GRAD / JTJP modes of k_eg_pass / k_eg_jtjp, 64 in k_eg_tile<1024>, 16 in the COLNORM
mode and in k_eg_gradcol.  The tiled kernels merge a table when more than (slots - 16) of them are in use after a tile, so at most 16 survive a merge.  A wave that meets more
distinct keyframes than that between two merges adds straight into the workgroup's dense accumulator instead — a second code path that neighbouring voxels of a smooth scene
never take: they choose the same keyframes.

Whether a voxel is observed by a keyframe is decided by ONE depth pixel (observe_device.hpp: d > 0 at the rounded projection).  Zeroing a random subset of depth pixels per
keyframe ("speckle") therefore gives neighbouring voxels unrelated keyframe sets, while the luminance stays dense and the rows valid.  A wave is 64 consecutive entries of the
work list, so
  * >= 33 distinct keyframes in a group of 64 entries force the branch in the 32-slot kernels (at most 16 slots are taken when the group starts: 17 or more do not fit), and
  * >= 65 force it in k_eg_tile<1024>."""
import numpy as np

import helpers

SLOTS_32, SLOTS_64 = 33, 65       # distinct keyframes per 64-entry group that guarantee the branch (never lower them: they are the guarantee, not a measurement)


def _speckled_scene(seed, K, keep):
    sc = dict(helpers.small_scene(radius_vox=10, width=96, height=72, levels=1, pose_noise=(0.01, 0.02), lum_noise=0.02, seed=seed, K=K))
    rng = np.random.default_rng(seed + 1)
    for fr in sc["frames"]:
        d = fr["depth"][0]
        d[rng.random(d.shape) >= keep] = 0
    return sc


def scene_diverse(seed=21):
    """Scene D: 256 keyframes, 6 % of the depth pixels kept.  Returns (scene, overrides of helpers.oracle_cfg)."""
    return _speckled_scene(seed, 256, 0.06), dict(iterations=1, fix_distortion=1, cg_fixed_iterations=-1)


def scene_rejecting(seed=21):
    """Scene R: 96 keyframes, 15 % of the depth pixels kept, regularisers weighted 1.0: the trust-region loop rejects its first attempts, so the speculative systems of the
    damping ladder decide the result.  Returns (scene, overrides of helpers.oracle_cfg)."""
    return _speckled_scene(seed, 96, 0.15), dict(iterations=1, fix_distortion=1, cg_fixed_iterations=-1, lambda_r0=1.0, lambda_r1=1.0, lambda_s0=1.0, lambda_s1=1.0)


def distinct_per_group(frames_of_entry, group=64):
    """frames_of_entry: [entries][slots] keyframe of every row slot in work-list order (debug_eg_rows()[0][work_list]), -1 = empty.  Returns the number of distinct keyframes of
    every group of `group` consecutive entries (the last one may be shorter)."""
    f = np.asarray(frames_of_entry)
    return np.array([len(np.setdiff1d(np.unique(f[a:a + group]), [-1])) for a in range(0, f.shape[0], group)], np.int64)


def group_shares(frames_of_entry):
    """share of the 64-entry groups that reach SLOTS_32 and SLOTS_64 distinct keyframes"""
    n = distinct_per_group(frames_of_entry)
    return float((n >= SLOTS_32).mean()), float((n >= SLOTS_64).mean())


def brick_order(keys, active):
    """A proxy for the device's work-list order where there is no device: the active voxels (visit indices) sorted by 4^3 brick, then inside the brick."""
    idx = np.nonzero(active)[0]
    k = np.asarray(keys)[idx].astype(np.int64); b = k >> 2; r = k & 3
    return idx[np.lexsort((r[:, 0], r[:, 1], r[:, 2], b[:, 0], b[:, 1], b[:, 2]))]


def oracle_frames_by_voxel(pv, slots=8):
    """the oracle's Eg rows as the [N][slots] keyframe table of debug_eg_rows (-1 = empty)"""
    v, f, _, _, _ = pv.eg(with_jacobian=False)
    out = np.full((pv.N, slots), -1, np.int32); fill = np.zeros(pv.N, np.int64)
    for vi, fi in zip(v.tolist(), f.tolist()):
        out[vi, fill[vi]] = fi; fill[vi] += 1
    return out


def pose_share_above(y, K, tol):
    """share of the 6K pose entries of a [sdf N | albedo N | poses 6K | intr 4 | dist 5] vector whose magnitude exceeds 100 x tol: a dropped or misplaced wave sum of
    such an entry is far outside the tolerance"""
    p = np.abs(np.asarray(y)[-(6 * K + 9):-9])
    return float((p > 100.0 * tol).mean())


BUILDERS = {"D": scene_diverse, "R": scene_rejecting}


def oracle_case(O, name, seed=21):
    """Scene `name` prepared on the oracle: the input state (grid `g`, frames, exported arrays, lighting) and the result of ONE outer iteration from it (`ref`, `intr`, `dist`,
    `poses`, `stats`).  The caller frees g and fr."""
    sc, kw = BUILDERS[name](seed)
    g, fr, arrays, vsh, thres = helpers.oracle_setup(O, sc)
    ocfg = helpers.oracle_cfg(O, thres, **kw)
    case = dict(name=name, sc=sc, kw=kw, g=g, fr=fr, arrays=arrays, vsh=vsh, thres=thres, ocfg=ocfg)
    rc, case["intr"], case["dist"], case["poses"], case["stats"], case["ref"] = oracle_run(O, case)
    assert rc == 0
    return case


def oracle_run(O, case, field_eps=0.0, seed=11):
    """one outer iteration of the oracle from the case's input fields, optionally perturbed by field_eps (relative, seeded normal draws)"""
    sc, a0 = case["sc"], case["arrays"]
    g2 = O.Grid.from_voxels(sc["voxel_size"], sc["keys"], sc["sdf"], sc["weight"], sc["color"]); g2.clear_outside_shell(case["thres"])
    s, a = a0["sdf_refined"], a0["albedo"]
    if field_eps != 0.0:
        rng = np.random.default_rng(seed)
        s = s * (1.0 + field_eps * rng.standard_normal(len(s))); a = a * (1.0 + field_eps * rng.standard_normal(len(a)))
    g2.import_fields(sdf_refined=s, albedo=a)
    rc, intr, dist, poses, stats = O.optimize(g2, case["fr"], case["ocfg"], sc["intr"], sc["dist"], sc["poses"], case["vsh"])
    ref = g2.export(); g2.free()
    return rc, intr, dist, poses, stats, ref


def oracle_envelope(O, case):
    """The oracle's own spread under a 1e-7 relative perturbation of its input fields (the conditioning envelope of tests/test_gpu_levels.py): max |change| of the refined
    SDF, the albedo, the intrinsics and the poses over four perturbed re-runs.  A re-run whose accept sequence differs is a different trajectory, not a measure of
    conditioning: not counted."""
    s0 = case["stats"][0]; seq = list(s0.accepted[:s0.n_attempts])
    env = dict(sdf_refined=0.0, albedo=0.0, intr=0.0, poses=0.0)
    for eps, seed in ((1e-7, 11), (-1e-7, 11), (1e-7, 12), (-1e-7, 12)):
        rc, intr, _, poses, st, per = oracle_run(O, case, eps, seed)
        if rc != 0 or list(st[0].accepted[:st[0].n_attempts]) != seq:
            continue
        for k in ("sdf_refined", "albedo"):
            env[k] = max(env[k], float(np.abs(per[k] - case["ref"][k]).max()))
        env["intr"] = max(env["intr"], float(np.abs(intr - case["intr"]).max())); env["poses"] = max(env["poses"], float(np.abs(poses - case["poses"]).max()))
    return env


def groups_with_rows(frames_of_entry, group=64):
    """which groups of `group` consecutive entries own at least one Eg row (the waves that run the row loop: the work list keeps the entries that cannot own rows at the
    back of every 512-entry block, k_partition_blocks, and waves made of them skip their row stream)"""
    f = np.asarray(frames_of_entry)
    return np.array([bool((f[a:a + group] >= 0).any()) for a in range(0, f.shape[0], group)])
