"""The numpy statement of i3d_fusion_extract_mesh: marching cubes over a fusion volume given as arrays, welded, cleaned and ordered as the
definition says.  Written from the definition and from the expressions it cites (k_mc_emit's vertex, MarchingCubes::interpolate, removeDegenerateFaces), every fp32
operation rounded on its own (numpy float32 arithmetic never contracts).

    mesh(vol, vs, tables, min_weight=0.0) -> dict(vertices [nv,3] f32, colors [nv,3] u8, faces [nf,3] i32, stats, soup_positions [T,3,3], soup_colors [T,3,3],
                                                  vertex_code [nv], vertex_owner [nv,3], direction_colour_conflicts)

vol = dict(keys [n,3], sdf [n], weight [n], color [n,3]) in any order with distinct keys; tables = (ntri [256], tri [256,16]) of i3d_mc_tables.

The weld.  Every triangle corner is NAMED (owner voxel, code).  A corner that lies on a lattice point is that voxel's code 0.  Any other lies on a cell edge; its owner
is the edge's lower voxel and its code 1, 2, 3 for the +x, +y, +z edge.  Cells walk their edges 0, 1, 4, 5 downwards (upper corner -> lower corner) while the cells next
to them walk the same edge upwards, and the interpolation v0 + mu (v1 - v0) is not symmetric in its last bit: where the downward walk gives another coordinate than the
upward one, the downward corner is a vertex of its own, code 4 (x) or 5 (y).  Named this way, two corners have the same name exactly when they have the same position
(+0 == -0) - the reference's weld, merge() of host/mesh.cpp - and mesh() asserts that on every volume it meshes by welding by position as well."""
import numpy as np

OFFSET = 1 << 20
F = np.float32
EA = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3])
EB = np.array([1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7])
CORNER = np.array([[1, 1, 0], [1, 0, 0], [0, 0, 0], [0, 1, 0], [1, 1, 1], [1, 0, 1], [0, 0, 1], [0, 1, 1]], np.int64)      # the reference's numbering
CODES = 6
STATS = ("stored", "valid_cells", "surface_cells", "raw_triangles", "vertices", "corner_vertices", "faces", "degenerate_removed", "rounded_corner_occurrences")


def pack(keys):
    """fusion_hash::pack_key: z, then y, then x"""
    k = np.asarray(keys, np.int64) + OFFSET
    return (k[..., 2] << 42) | (k[..., 1] << 21) | k[..., 0]


def lerp(t0, t1, v0, v1):
    """MarchingCubes::interpolate on one component, fp32, elementwise"""
    t0, t1, v0, v1 = (np.asarray(a, F) for a in np.broadcast_arrays(t0, t1, v0, v1))
    with np.errstate(all="ignore"):
        mu = (F(0) - t0) / (t1 - t0)
        mu = np.maximum(np.minimum(mu, F(1)), F(0))
        r = v0 + mu * (v1 - v0)
        r = np.where(np.abs(t0 - t1) < F(0.00001), v0, r)
        r = np.where(np.abs(F(0) - t1) < F(0.00001), v1, r)
        r = np.where(np.abs(F(0) - t0) < F(0.00001), v0, r)
    return r.astype(F)


def early(t0, t1):
    """one of interpolate's three early returns is taken"""
    with np.errstate(all="ignore"):
        return (np.abs(F(0) - t0) < F(0.00001)) | (np.abs(F(0) - t1) < F(0.00001)) | (np.abs(t0 - t1) < F(0.00001))


def color8(x):
    """(unsigned char)(x * 255.0f)"""
    return (np.asarray(x, F) * F(255)).astype(np.int64).astype(np.uint8)


def degenerate(a, b, c):
    """removeDegenerateFaces' area test on positions [T,3] fp32: the area is 0, NaN or inf"""
    with np.errstate(all="ignore"):
        e0 = (c - a).astype(F); e1 = (c - b).astype(F)
        cr0 = (e0[:, 1] * e1[:, 2]).astype(F) - (e0[:, 2] * e1[:, 1]).astype(F)
        cr1 = (e0[:, 2] * e1[:, 0]).astype(F) - (e0[:, 0] * e1[:, 2]).astype(F)
        cr2 = (e0[:, 0] * e1[:, 1]).astype(F) - (e0[:, 1] * e1[:, 0]).astype(F)
        area = np.sqrt((cr0 * cr0 + (cr1 * cr1 + cr2 * cr2)).astype(F)).astype(np.float64)
    return (area == 0.0) | ~np.isfinite(area)


def _empty(stats):
    z = np.zeros((0, 3))
    return dict(vertices=z.astype(F), colors=z.astype(np.uint8), faces=z.astype(np.int32), stats=stats, soup_positions=np.zeros((0, 3, 3), F),
                soup_colors=np.zeros((0, 3, 3), np.uint8), vertex_code=np.zeros(0, np.int64), vertex_owner=z.astype(np.int64), direction_colour_conflicts=0)


def mesh(vol, vs, tables, min_weight=0.0):
    ntri, tri = np.asarray(tables[0]).astype(np.int64), np.asarray(tables[1]).astype(np.int64).reshape(256, 16)
    vs = F(vs); min_weight = F(min_weight)
    keys = np.asarray(vol["keys"], np.int64).reshape(-1, 3)
    w = np.asarray(vol["weight"], F); stored = w != 0
    stats = dict.fromkeys(STATS, 0)
    order = np.flatnonzero(stored)[np.argsort(pack(keys[stored]), kind="stable")]
    K = keys[order]; S = np.asarray(vol["sdf"], F)[order]; W = w[order]; C = np.asarray(vol["color"], np.uint8).reshape(-1, 3)[order]
    P = pack(K); n = len(P)
    assert np.all(np.diff(P) > 0), "fusion_mesh_twin: the keys are not distinct"
    stats["stored"] = n
    if n == 0:
        return _empty(stats)
    # ---- item 1: the cell of every list entry --------------------------------------------------------------------------------------------------------------
    ck = K[:, None, :] + CORNER[None]                                            # [n, 8, 3]
    cp = pack(ck); at = np.minimum(np.searchsorted(P, cp), n - 1)
    found = (P[at] == cp) & np.all(ck < OFFSET, -1)
    with np.errstate(invalid="ignore"):
        ok = found & (W[at] >= min_weight) & np.isfinite(S[at])
    valid = ok.all(1)
    cs = S[at]                                                                    # [n, 8]
    idx = ((cs < 0).astype(np.int64) << np.arange(8)).sum(1)
    surface = valid & (idx != 0) & (idx != 255)
    stats["valid_cells"] = int(valid.sum()); stats["surface_cells"] = int(surface.sum())
    cells = np.flatnonzero(surface)
    # ---- item 2 / 5: the triangles, cells in ascending key, a cell's triangles in table order --------------------------------------------------------------
    reps = ntri[idx[cells]]
    tcell = np.repeat(cells, reps)
    tk = np.concatenate([np.arange(r) for r in reps]) if len(reps) else np.zeros(0, np.int64)
    T = len(tcell); stats["raw_triangles"] = T
    if T == 0:
        return _empty(stats)
    e = tri[idx[tcell][:, None], 3 * tk[:, None] + np.arange(3)[None]]            # [T, 3]
    assert e.min() >= 0
    a, b = EA[e], EB[e]
    ci = tcell[:, None]
    s1, s2 = cs[ci, a], cs[ci, b]
    ka, kb = ck[ci, a], ck[ci, b]                                                 # [T, 3, 3]
    va, vb = ka.astype(F) * vs, kb.astype(F) * vs
    # ---- item 3: the soup vertex -------------------------------------------------------------------------------------------------------------------------------
    pos = lerp(s1[..., None], s2[..., None], va, vb)
    inv = F(1.0) / F(255.0)
    ca, cb = C[at[ci, a]].astype(F) * inv, C[at[ci, b]].astype(F) * inv
    col = color8(lerp(s1[..., None], s2[..., None], ca, cb))
    # ---- item 4: names -------------------------------------------------------------------------------------------------------------------------------------------
    at_a, at_b = np.all(pos == va, -1), np.all(pos == vb, -1)
    assert not np.any(at_a & at_b)
    corner = at_a | at_b
    stats["rounded_corner_occurrences"] = int((corner & ~early(s1, s2)).sum())
    axis = np.where(e >= 8, 2, np.where(e & 1, 0, 1))
    down = (e < 8) & ((e & 2) == 0)
    take = lambda x: np.take_along_axis(x, axis[..., None], -1)[..., 0]
    up_pos = lerp(s2, s1, take(vb), take(va))                                     # the same edge walked upwards (meaningful where down)
    twin = down & (up_pos != take(pos))
    code = np.where(corner, 0, np.where(twin, axis + 4, axis + 1))
    owner = np.where(corner, np.where(at_a, at[ci, a], at[ci, b]), np.where(down, at[ci, b], at[ci, a]))
    name = owner * CODES + code                                                   # [T, 3]
    # the reference's weld: by position.  The same names <=> the same positions
    pz = (pos + F(0)).reshape(-1, 3)                                              # -0 -> +0
    _, by_pos = np.unique(pz.view(np.uint32), axis=0, return_inverse=True)
    by_pos = by_pos.reshape(-1)
    uname, first, by_name = np.unique(name.reshape(-1), return_index=True, return_inverse=True)
    by_name = by_name.reshape(-1)
    pairs = np.unique(np.stack([by_pos, by_name], 1), axis=0)
    assert len(pairs) == len(uname) == by_pos.max() + 1, "fusion_mesh_twin: the weld by (owner, code) is not the weld by position"
    # ---- vertices in ascending (owner key, code) -----------------------------------------------------------------------------------------------------------------
    vcode = uname % CODES; vown = uname // CODES
    vertices = pos.reshape(-1, 3)[first]
    # colour: a corner vertex its owner's stored colour; an edge vertex the interpolated colour of ITS direction (codes 1..3 upwards, 4..5 downwards)
    up_col = color8(lerp(s2[..., None], s1[..., None], cb, ca))
    own_dir = np.where((down & ~twin)[..., None], up_col, col).reshape(-1, 3)
    colors = np.where((vcode == 0)[:, None], color8(C[vown].astype(F) * inv), own_dir[first])
    conflicts = int(np.any(col.reshape(-1, 3) != colors[by_name], 1)[(code.reshape(-1) != 0)].sum())
    early_corner = (corner & early(s1, s2)).reshape(-1)
    assert np.array_equal(col.reshape(-1, 3)[early_corner], colors[by_name][early_corner])      # item 4: every early-return occurrence computes the corner's colour
    stats["vertices"] = len(uname); stats["corner_vertices"] = int((vcode == 0).sum())
    # ---- item 6: faces ---------------------------------------------------------------------------------------------------------------------------------------------
    f = by_name.reshape(-1, 3)
    drop = (f[:, 0] == f[:, 1]) | (f[:, 0] == f[:, 2]) | (f[:, 1] == f[:, 2])
    drop |= degenerate(pos[:, 0], pos[:, 1], pos[:, 2])
    faces = f[~drop].astype(np.int32)
    stats["faces"] = len(faces); stats["degenerate_removed"] = int(drop.sum())
    assert len(uname) <= 2 ** 31 - 1 and 3 * len(faces) <= 2 ** 31 - 1
    return dict(vertices=vertices, colors=colors, faces=faces, stats=stats, soup_positions=pos, soup_colors=col, vertex_code=vcode, vertex_owner=K[vown],
                direction_colour_conflicts=conflicts)


def weld_by_position(soup_positions, soup_colors):
    """merge() + removeDegenerateFaces of host/mesh.cpp in plain Python: vertices in order of first appearance, the first appearance's colour"""
    index = {}; V = []; Cc = []; faces = []
    p = (np.asarray(soup_positions, F) + F(0)).reshape(-1, 3); c = np.asarray(soup_colors, np.uint8).reshape(-1, 3)
    ids = []
    for i in range(len(p)):
        k = p[i].tobytes()
        if k not in index:
            index[k] = len(V); V.append(p[i]); Cc.append(c[i])
        ids.append(index[k])
    V = np.array(V, F).reshape(-1, 3); Cc = np.array(Cc, np.uint8).reshape(-1, 3); ids = np.array(ids, np.int64).reshape(-1, 3)
    drop = (ids[:, 0] == ids[:, 1]) | (ids[:, 0] == ids[:, 2]) | (ids[:, 1] == ids[:, 2])
    if len(ids):
        drop |= degenerate(V[ids[:, 0]], V[ids[:, 1]], V[ids[:, 2]])
    return V, Cc, ids[~drop].astype(np.int32)
