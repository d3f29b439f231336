"""-m gpu: the I3D_* switches of the solver are read at the top of every assemble (read_switches, solver.cpp), never cached per process: a switch changed
between two optimize calls of ONE context takes effect at the next call, and changing it back gives the first answer back.

One context, a small scene (K = 6 keyframes, 5 observation slots, fifteen 512-entry tiles, no keyframe table near its capacity), every run restarted from the
same uploaded grid, lighting and camera, two outer iterations, the bit-reproducible mode (the default on one rank):
  * I3D_LADDER=1 | unset | I3D_LADDER=1 (the 512-entry tile geometry throughout: a context keeps last call's row density, which would otherwise pick the geometry
    of the first outer iteration differently in the first and in the third run): ladder batches 0, > 0, 0, and the first and the third run equal byte for byte;
  * I3D_EGT_TILE=1024 | unset | I3D_EGT_TILE=1024, all under I3D_LADDER=1: the first and the third run equal byte for byte.  No probe of the library reports
    the plan's geometry, so the geometry of the middle run is not asserted."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


def switch_scene(O):
    sc = helpers.small_scene(seed=11, radius_vox=12, K=6)
    g, fr, arrays, vsh, thres = helpers.oracle_setup(O, sc)
    cfg = helpers.gpu_cfg(helpers.oracle_cfg(O, thres, iterations=2, num_observations=5))
    return sc, arrays, vsh, cfg


def restart(ctx, sc, arrays, vsh):
    ctx.set_grid(sc["voxel_size"], arrays["keys"], arrays["sdf"], arrays["sdf_refined"], arrays["albedo"], arrays["weight"], arrays["color"])
    ctx.set_camera(sc["intr"], sc["dist"], sc["poses"])
    ctx.set_voxel_sh(vsh)


def _stats(st):
    return [(s.num_attempts, list(s.step_accepted[:s.num_attempts]), list(s.pcg_iterations[:s.num_attempts]), s.cost_initial, s.cost_final, s.final_radius, s.termination,
             list(s.rows)) for s in st]


@pytest.fixture(scope="module")
def setup(oracle):
    sc, arrays, vsh, cfg = switch_scene(oracle)
    ctx = helpers.gpu_context(sc, arrays, vsh)
    yield sc, arrays, vsh, cfg, ctx
    ctx.close()


def _run(setup, monkeypatch, env):
    sc, arrays, vsh, cfg, ctx = setup
    for k in ("I3D_LADDER", "I3D_EGT_TILE", "I3D_DETERMINISTIC"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    restart(ctx, sc, arrays, vsh)
    before = ctx.debug_ladder_stats()["batches"]
    st = ctx.optimize(cfg)
    sdf, alb = ctx.get_grid(); cam = ctx.get_camera()
    return dict(stats=_stats(st), bytes=(sdf.tobytes(), alb.tobytes()) + tuple(np.asarray(x).tobytes() for x in cam), batches=ctx.debug_ladder_stats()["batches"] - before,
                sizes=ctx.problem_sizes())


def test_ladder_switch_is_read_at_every_call(setup, monkeypatch):
    a = _run(setup, monkeypatch, {"I3D_LADDER": "1", "I3D_EGT_TILE": "512"})
    b = _run(setup, monkeypatch, {"I3D_EGT_TILE": "512"})
    c = _run(setup, monkeypatch, {"I3D_LADDER": "1", "I3D_EGT_TILE": "512"})
    print("active / eg rows:", a["sizes"]["active"], a["sizes"]["eg"], "batches:", a["batches"], b["batches"], c["batches"])
    assert a["sizes"]["active"] >= 3 * 512 and sum(s[0] for s in a["stats"]) >= 2
    assert a["batches"] == 0 and b["batches"] > 0 and c["batches"] == 0
    assert a["stats"] == c["stats"] and a["bytes"] == c["bytes"]


def test_tile_switch_is_read_at_every_call(setup, monkeypatch):
    a = _run(setup, monkeypatch, {"I3D_LADDER": "1", "I3D_EGT_TILE": "1024"})
    b = _run(setup, monkeypatch, {"I3D_LADDER": "1"})
    c = _run(setup, monkeypatch, {"I3D_LADDER": "1", "I3D_EGT_TILE": "1024"})
    assert a["batches"] == 0 and b["batches"] == 0 and c["batches"] == 0
    assert a["stats"] == c["stats"] and a["bytes"] == c["bytes"]
