"""-m gpu: the one slot list of a fusion handle under all four of its users in turn.  finish, merge, register_volume and extract_mesh
build "the selected slots of the table as a sorted list" in one set of grown-only buffers of the handle; each list has another length, another selector and
another payload, and the table grows between them.  On one handle the calls run in an order that follows a list of n entries by a longer one and by a shorter
one, and after every call the output is compared bit for bit with the same call on freshly built handles brought to the same state (the merges so far replayed):
meshes, the selection, poses and statistics, the merge statistics and the table read by key, the exported records (their order is the order of the ranks).

The scene is the "textured" one of test_gpu_fusion_merge.py (3 frames at 96 x 72, sphere radius 10 voxels); every volume starts with the smallest table, 4096
slots."""
import math

import numpy as np
import pytest

import fusion_cases as FC
from intrinsic3d_amd import binding as B

pytestmark = pytest.mark.gpu

AXIS = np.array([0.3, -0.8, 0.52])
POSE = np.concatenate([AXIS / np.linalg.norm(AXIS) * math.radians(20.0), [0.0131, -0.0207, 0.0049]])     # general: oblique, no lattice translation
START = np.array([0.01, -0.02, 0.015, 0.002, -0.001, 0.0015])                                           # where the registrations start
MIN_SLOTS = 4096

# the issue's order: mesh before merge; a list is followed by a shorter one (mesh -> register -> merge) and by a longer one (merge -> mesh, register2 -> export)
MESH_FIRST = ("mesh", "register", "selection", "merge", "merge_again", "mesh", "register_stride2", "export")
MERGE_FIRST = ("merge", "mesh", "register", "merge_again", "selection", "export")
MERGES = ("merge", "merge_again")


@pytest.fixture(scope="module")
def scene():
    sc, fr = FC.textured_frames(seed=5, K=3, radius=10, w=96, h=72)
    intr = sc["intr"].astype(np.float32)
    return dict(vs=float(sc["voxel_size"]), frames=[(d, intr, bgr, T, 2) for d, bgr, T in fr])


def _fuse(scene, frames):
    f = B.Fusion(scene["vs"], 0.1, 10.0, initial_capacity=1)
    assert f.info()["capacity"] == MIN_SLOTS
    for d, intr, bgr, T, er in frames:
        f.integrate(d, intr, bgr, intr, T, er)
    return f


def _pair(scene):
    """A: the three frames, a table loaded just below the growth threshold, so that the merge grows it; B: the third frame alone, a smaller volume and table"""
    return _fuse(scene, scene["frames"]), _fuse(scene, scene["frames"][2:3])


@pytest.fixture(scope="module")
def box(scene):
    """a dense box of keys that holds every voxel A stores after the merges"""
    A, Bv = _pair(scene)
    with A, Bv:
        A.merge(Bv, POSE)
        A.finish(0); keys = A.export()["keys"]
    lo, hi = keys.min(0).astype(np.int64) - 12, keys.max(0).astype(np.int64) + 13
    return np.ascontiguousarray(np.stack(np.meshgrid(*[np.arange(lo[a], hi[a], dtype=np.int32) for a in range(3)], indexing="ij"), -1).reshape(-1, 3))


def _call(A, Bv, step, box):
    """one step on the pair, as a flat dict of what it returned"""
    if step == "mesh":
        v, c, f, st = A.extract_mesh(stats=True)
        return dict(mesh_vertices=v, mesh_colors=c, mesh_faces=f, capacity=A.info()["capacity"], **st)
    if step in ("register", "register_stride2"):
        pose, st = A.register_volume(Bv, START, **(dict(stride=2) if step == "register_stride2" else {}))
        return dict(pose=pose, **st)
    if step == "selection":
        return Bv.debug_register_volume_selection()
    if step in MERGES:
        st = A.merge(Bv, POSE)
        return dict(st, capacity=A.info()["capacity"], **{"table_" + k: v for k, v in A.debug_voxels(box).items()})
    assert step == "export"
    return A.export()


def _same(got, want, where):
    assert got.keys() == want.keys(), where
    for k in got:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (where, k)


def _run(scene, box, order):
    A, Bv = _pair(scene)
    outs = []
    with A, Bv:
        for i, step in enumerate(order):
            got = _call(A, Bv, step, box)
            FA, FB = _pair(scene)                            # fresh handles at the same state: the merges so far, nothing else
            with FA, FB:
                for earlier in order[:i]:
                    if earlier in MERGES:
                        FA.merge(FB, POSE)
                _same(got, _call(FA, FB, step, box), (order, i, step))
            outs.append(got)
    return outs


def test_mesh_before_merge(scene, box):
    outs = dict(zip(["mesh0", "register", "selection", "merge", "merge_again", "mesh", "register_stride2", "export"], _run(scene, box, MESH_FIRST)))
    # the sequence is the one meant: the merge inserts and the table grows under the list, the second merge inserts nothing, and the lists differ in length
    assert outs["merge"]["allocated"] > 0 and outs["merge"]["aligned"] == 0 and outs["merge_again"]["allocated"] == 0
    assert outs["merge"]["capacity"] > outs["mesh0"]["capacity"] > MIN_SLOTS
    assert outs["mesh"]["stored"] > outs["mesh0"]["stored"] > outs["register"]["selected"] > outs["register_stride2"]["selected"] > 0
    assert len(outs["selection"]["sdf"]) == outs["register"]["selected"] and len(outs["export"]["sdf"]) > 0
    assert outs["mesh0"]["faces"] > 0 and outs["register"]["inliers"] > 0


def test_merge_before_mesh(scene, box):
    outs = dict(zip(MERGE_FIRST, _run(scene, box, MERGE_FIRST)))
    assert outs["merge"]["allocated"] > 0 and outs["merge_again"]["allocated"] == 0 and outs["mesh"]["stored"] > outs["register"]["selected"] > 0
    A, Bv = _pair(scene)
    with A, Bv:                                              # the same state reached with a mesh first gives the same mesh
        _call(A, Bv, "mesh", box); _call(A, Bv, "merge", box)
        _same(_call(A, Bv, "mesh", box), outs["mesh"], "mesh -> merge -> mesh against merge -> mesh")
