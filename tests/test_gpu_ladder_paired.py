"""-m gpu: the paired launch of the multi-system operator pass (tile_pass_mr.hip, PAIR; pcg.cpp pcg_solve_ladder).

A PCG pass of the damping ladder with 4, 5 or 6 live systems is two groups of at most three.  As two launches each group streams every stored row from HBM; the paired
launch issues both groups at once and places the two workgroups that own the same tile range on one XCD, so that the second read of a row block comes out of a cache.
Every logical workgroup keeps its tile range, the order inside it and its slot in every per-workgroup partial array, so NOTHING about the result may change: in the
bit-reproducible mode fields, camera, costs, radii, attempts and PCG counts must be equal BIT FOR BIT between the paired launch (the default) and the two-launch path
(I3D_LADDER_PAIR=0).

The scene: the bench slice (bench_slice.py), outer iterations from the state its second iteration starts from — the iterations with the rejected attempts.
Without history the batches grow 2 -> 4 (four live systems: 2 + 2); the next iteration opens with a batch as deep as the attempts of the one before (five: 3 + 2), and
the one behind it with six (3 + 3): the batch depth follows the history of the context (solver.cpp lm_solve), so a pass with six live systems cannot occur before the
THIRD iteration of a context: the comparison is made after two iterations (4 and 5 live systems) and again after three (4, 5 and 6), each time over every iteration's
attempts, accept sequence, PCG counts, costs and radii and over the final fields and camera.  That the run really went through passes of every width, and that they were single launches, is asserted from the library's own pass counters
(i3d_debug_ladder_passes): the test cannot pass by never taking the new path."""
import numpy as np
import pytest

import helpers
from bench_slice import bench_cfg, second_iteration_start, stats
from bench_slice import slice_setup  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _run_n(S, iterations):
    sc2, arrays = second_iteration_start(S)
    cfg = helpers.gpu_cfg(bench_cfg(S["O"], S["thres"], -1, second=True)); cfg.iterations = iterations
    ctx = helpers.gpu_context(sc2, arrays, S["vsh"])
    st = ctx.optimize(cfg); sdf, alb = ctx.get_grid(); cam = ctx.get_camera(); lad = ctx.debug_ladder_stats(); lad.update(ctx.debug_ladder_passes()); ctx.close()
    return st, sdf, alb, cam, lad


def _both(S, monkeypatch, iterations):
    monkeypatch.setenv("I3D_EGT_TILE", "512"); monkeypatch.setenv("I3D_DETERMINISTIC", "1")
    monkeypatch.setenv("I3D_LADDER", "6"); monkeypatch.setenv("I3D_LADDER_GROUP", "3"); monkeypatch.setenv("I3D_LADDER_MR", "1")
    monkeypatch.setenv("I3D_LADDER_PAIR", "0")
    two = _run_n(S, iterations)
    monkeypatch.setenv("I3D_LADDER_PAIR", "1")
    pair = _run_n(S, iterations)
    st1, s1, a1, c1, l1 = two; st2, s2, a2, c2, l2 = pair
    print(f"\n[paired launch, {iterations} iterations] attempts {[s.num_attempts for s in st1]}, PCG counts {[list(s.pcg_iterations[:s.num_attempts]) for s in st1]}; passes by live systems "
          f"{l1['live']}; two launches: {l1['row_streams']} streams for {l1['system_passes']} system passes, {l1['paired']} paired; paired: {l2['row_streams']} streams, {l2['paired']} paired")
    assert l2["live"] == l1["live"] and l1["depth"] == 6 and l2["depth"] == 6 and l1["resyncs"] == 0 and l2["resyncs"] == 0, (l1, l2)
    # every pass with more than three live systems is ONE stream of the rows on the new path and two on the old one; nothing else about the streams moved
    wide = sum(l1["live"][4:])
    assert l1["paired"] == 0 and l2["paired"] == wide, (l1, l2)
    assert l2["system_passes"] == l1["system_passes"] and l2["batches"] == l1["batches"] and l2["row_streams"] == l1["row_streams"] - wide, (l1, l2)
    # nothing else changed: attempts, accept sequence, PCG counts, costs, radii (stats), fields and camera
    assert stats(st1) == stats(st2), (stats(st1), stats(st2))
    diffs = {"sdf": float(np.abs(s1 - s2).max()), "albedo": float(np.abs(a1 - a2).max()), "intr": float(np.abs(c1[0] - c2[0]).max()), "dist": float(np.abs(c1[1] - c2[1]).max()),
             "poses": float(np.abs(c1[2] - c2[2]).max())}
    assert np.array_equal(s1, s2) and np.array_equal(a1, a2) and all(np.array_equal(x, y) for x, y in zip(c1, c2)), diffs
    return l1["live"]


def test_paired_launch_is_the_two_launch_path_bit_for_bit(slice_setup, monkeypatch):
    live2 = _both(slice_setup, monkeypatch, 2)
    assert live2[4] > 0 and live2[5] > 0, live2          # 2 + 2 and 3 + 2
    live3 = _both(slice_setup, monkeypatch, 3)
    assert all(live3[n] > 0 for n in (4, 5, 6)), live3   # ... and 3 + 3
