"""The numpy statement of the device stages of the SH lighting estimate, written from the definitions the kernels cite
(lighting_svsh.cpp:196-253, subvolumes.cpp:164-295, math.cpp:74-128, operators.cpp:142-147), not from the kernels' structure: no tiles, chunks,
slices or sorted lists here.  fp32 quantities are np.float32 arrays, so every operation rounds once; the sums are exact (error-free products,
math.fsum).  tests/test_sh_twin_cpu.py pins this file against the oracle before tests/test_gpu_sh_stages.py lets it judge the device.

A grid is a dict: voxel_size, keys [N, 3] int32, sdf, sdf_refined, albedo [N] float64, weight [N] float32, color [N, 3] uint8 (the channel order of
set_grid), and optionally truncation (default float32(voxel_size) * 5)."""
import math

import numpy as np

F = np.float32
_B = 1 << 20
RING6 = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int64)                  # algorithms.cpp:75-91
CORNERS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]], np.int64)   # math.cpp:103-128


def pack(idx):
    """21 bits per coordinate, offset 2^20, x lowest: ascending packed order is the order i3d_estimate_sh reports the subvolumes in"""
    i = np.asarray(idx, np.int64)
    assert np.all(np.abs(i) < _B)
    return (i[..., 0] + _B) | ((i[..., 1] + _B) << 21) | ((i[..., 2] + _B) << 42)


class _Lookup:
    """position of an integer triple in a list of distinct triples, -1 if absent"""

    def __init__(self, triples):
        c = pack(triples); self.order = np.argsort(c, kind="stable"); self.codes = c[self.order]
        assert np.all(np.diff(self.codes) > 0), "duplicate triples"

    def __call__(self, q):
        c = pack(q)
        if self.codes.size == 0:
            return np.full(c.shape, -1, np.int64)
        p = np.minimum(np.searchsorted(self.codes, c), self.codes.size - 1)
        return np.where(self.codes[p] == c, self.order[p], -1)


def truncation(grid):
    return F(grid["truncation"]) if grid.get("truncation") is not None else F(grid["voxel_size"]) * F(5.0)


def subvolume_index(keys, vs, size):
    """Subvolumes::pointToIndex of voxelToWorld (subvolumes.cpp:263-295): floor((float(c) * vs) * (1.0f / size)), one fp32 rounding per operation"""
    world = np.asarray(keys).astype(F) * F(vs)
    inv = F(1.0) / F(size)
    return np.floor(world * inv).astype(np.int32)


def subvolume_set(keys, vs, size):
    """every stored voxel allocates its subvolume (subvolumes.cpp:211-237); [S, 3] in packed order.  size <= 0: one global volume"""
    if size <= 0:
        return np.zeros((1, 3), np.int32)
    idx = np.unique(subvolume_index(keys, vs, size), axis=0)
    return idx[np.argsort(pack(idx), kind="stable")]


def neighbours(grid):
    """[N, 3]: the positions of the +x, +y, +z neighbours in the voxel list, -1 = not stored"""
    look = _Lookup(grid["keys"]); k = np.asarray(grid["keys"], np.int64)
    return np.stack([look(k + RING6[0]), look(k + RING6[2]), look(k + RING6[4])], axis=1)


def forward_differences(grid, nb):
    """fp32 forward differences of the fp32 sdf_refined and their length sqrt(gx^2 + (gy^2 + gz^2)) (operators.cpp:58-77); NaN where a neighbour is missing"""
    f = np.asarray(grid["sdf_refined"], np.float64).astype(F)
    g = np.full((f.shape[0], 3), np.nan, F)
    for a in range(3):
        m = nb[:, a] >= 0
        g[m, a] = f[nb[m, a]] - f[m]
    with np.errstate(invalid="ignore"):
        length = np.sqrt(g[:, 0] * g[:, 0] + (g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]))
    return g, length


def in_shell(grid, thres):
    """the voxels that receive interpolated coefficients (lighting_svsh.cpp:93-110)"""
    return (np.asarray(grid["weight"]) > 0) & ~(np.abs(np.asarray(grid["sdf_refined"], np.float64)) > float(thres))


def eligible(grid, thres, nb=None):
    """the voxels of the data term (lighting_svsh.cpp:203-231)"""
    nb = neighbours(grid) if nb is None else nb
    w = np.asarray(grid["weight"]); alb = np.asarray(grid["albedo"], np.float64)
    ok = in_shell(grid, thres)
    for a in range(3):
        ok &= (nb[:, a] >= 0) & (w[np.maximum(nb[:, a], 0)] > 0)
    _, length = forward_differences(grid, nb)
    ok &= ~np.isnan(length) & (length != 0)
    ok &= ~np.isnan(alb) & (alb != 0.0)          # -0.0 == 0.0
    return ok


def features(grid, sel, nb=None):
    """of the voxels sel: ([n, 10] float64 = albedo * H(n) (shading.h:53-66 order: 1, y, z, x, xy, yz, -x^2 - y^2 + 2 z^2, xz, x^2 - y^2) and the luminance;
    [n] float64 weights sdfToWeight (operators.cpp:142-147))"""
    nb = neighbours(grid) if nb is None else nb
    g, length = forward_differences(grid, nb)
    n32 = g[sel] / length[sel][:, None]                                                # fp32 normalisation
    x, y, z = (n32[:, a].astype(np.float64) for a in range(3))
    a = np.asarray(grid["albedo"], np.float64)[sel]
    c = np.asarray(grid["color"])[sel].astype(F)
    lum = ((F(0.299) * c[:, 0] + F(0.587) * c[:, 1]) + F(0.114) * c[:, 2]) / F(255.0)  # color_util.cpp:41-52, lighting_svsh.cpp:233
    f = np.stack([a, a * y, a * z, a * x, a * (x * y), a * (y * z), a * ((-(x * x)) - (y * y) + 2.0 * (z * z)), a * (x * z), a * ((x * x) - (y * y)),
                  lum.astype(np.float64)], axis=1)
    tr = float(truncation(grid)); s = np.asarray(grid["sdf_refined"], np.float64)[sel]
    w = np.minimum(np.maximum(1.0 - np.minimum(np.abs(s), tr) / tr, 0.01), 1.0)
    return f, w


def _split(a):
    c = 134217729.0 * a; hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker)"""
    p = a * b; ah, al = _split(a); bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def gram(f, w, sub, S, fp32=False):
    """per subvolume: G = sum w [phi; I][phi; I]^T [S, 10, 10], sum w [S], A = sum w |f_i| |f_j| [S, 10, 10], run length [S].  The products are error-free and
    math.fsum adds exactly, so G carries one rounding (only w f_i's low part times f_j is rounded, at 2^-106 of the term).  fp32 = True accumulates a block the
    way a single-precision kernel would (a mutation of tests/test_sh_twin_cpu.py, never the reference)."""
    f = np.asarray(f, np.float64); w = np.asarray(w, np.float64); sub = np.asarray(sub)
    G = np.zeros((S, 10, 10)); A = np.zeros((S, 10, 10)); ws = np.zeros(S); n = np.zeros(S, np.int64)
    for s in range(S):
        m = sub == s; n[s] = int(m.sum())
        if n[s] == 0:
            continue
        fs, wv = f[m], w[m]
        ws[s] = math.fsum(wv.tolist())
        A[s] = np.einsum("v,vi,vj->ij", wv, np.abs(fs), np.abs(fs))
        if fp32:
            wf = (wv[:, None] * fs).astype(F)
            G[s] = np.cumsum(wf[:, :, None] * fs.astype(F)[:, None, :], axis=0, dtype=F)[-1]
            continue
        for i in range(10):
            p, e = _two_prod(wv, fs[:, i])
            for j in range(i, 10):
                p2, e2 = _two_prod(p, fs[:, j]); p3, e3 = _two_prod(e, fs[:, j])
                G[s, i, j] = G[s, j, i] = math.fsum(np.concatenate([p2, e2, p3, e3]).tolist())
    return G, ws, A, n


def gram_bound(A, n):
    """|G_dev - G| <= 4 (n_s + 32) 2^-53 A, entry by entry: a rounded product w f and one fused multiply-add per voxel and entry, n_s / 2048 + 1 chunk additions,
    a factor 4 for the unspecified order inside a matrix instruction"""
    return 4.0 * (np.asarray(n, np.float64)[:, None, None] + 32.0) * 2.0 ** -53 * A


def weight_bound(ws, n):
    return (np.asarray(n, np.float64) + 8.0) * 2.0 ** -53 * ws


def pairs(indices):
    """the directed 6-neighbour pairs (i, neighbour) between stored subvolumes, +x -x +y -y +z -z per i (lighting_svsh.cpp:258-289): [P, 2]"""
    idx = np.asarray(indices, np.int64); look = _Lookup(idx); out = []
    for d in range(6):
        k = look(idx + RING6[d]); i = np.nonzero(k >= 0)[0]
        out.append(np.stack([i, k[i], np.full(i.shape, d)], axis=1))
    p = np.concatenate(out)
    return p[np.lexsort((p[:, 2], p[:, 0]))][:, :2]


def interpolation_p(keys, vs, size, fused=False):
    """p = (float(c) * vs) * (1.0f / size) - 0.5f in fp32 (subvolumes.cpp:164-175).  fused = False rounds the product and the difference separately (the
    reference); fused = True rounds once, as a fused multiply-add does: the fp64 product of two fp32 numbers is exact, and so is the difference here."""
    world = np.asarray(keys).astype(F) * F(vs); inv = F(1.0) / F(size)
    if fused:
        return (world.astype(np.float64) * np.float64(inv) - 0.5).astype(F)
    return world * inv - F(0.5)


def corner_lookup(keys, vs, size, indices, fused=False):
    """[N, 8] positions of the eight corner subvolumes (-1 = missing) and their fp32 weights, in the corner order of math.cpp:103-128"""
    p = interpolation_p(keys, vs, size, fused)
    p0 = np.floor(p); wt = p - p0                                                    # p0 is an integer-valued fp32: (float)x0 is exact
    ax, ay, az = wt[:, 0], wt[:, 1], wt[:, 2]; one = F(1.0)
    w8 = np.stack([(one - ax) * (one - ay) * (one - az), ax * (one - ay) * (one - az), (one - ax) * ay * (one - az), (one - ax) * (one - ay) * az,
                   ax * ay * (one - az), (one - ax) * ay * az, ax * (one - ay) * az, ax * ay * az], axis=1)
    look = _Lookup(indices); base = p0.astype(np.int64)
    ids = np.stack([look(base + CORNERS[i]) for i in range(8)], axis=1)
    return ids, w8


def interpolate(keys, vs, size, indices, sh, shell, fused=False):
    """Subvolumes::interpolate + math::average (subvolumes.cpp:164-205, math.cpp:74-96) of the coefficients sh [S, 9] at every voxel of the mask shell, cast to
    fp32; exact zeros elsewhere.  Missing subvolumes and zero weights are skipped, the first term is assigned, the rest are added in fp64 (product rounded, then
    the sum), the result is scaled by double(1.0f / sum_w)."""
    keys = np.asarray(keys); sh = np.asarray(sh, np.float64); shell = np.asarray(shell, bool); N = keys.shape[0]
    out = np.zeros((N, 9), F)
    if size <= 0:
        out[shell] = sh[0].astype(F)
        return out
    ids, w8 = corner_lookup(keys, vs, size, indices, fused)
    o = np.zeros((N, 9)); sum_w = np.zeros(N, F)
    for i in range(8):
        m = (ids[:, i] >= 0) & (w8[:, i] != 0)
        term = w8[:, i].astype(np.float64)[:, None] * sh[np.maximum(ids[:, i], 0)]
        first = m & (sum_w == 0); rest = m & ~first
        o[first] = term[first]; o[rest] = o[rest] + term[rest]
        sum_w[m] = sum_w[m] + w8[m, i]
    nz = sum_w != 0
    o[nz] = o[nz] * (F(1.0) / sum_w[nz]).astype(np.float64)[:, None]
    out[shell] = o[shell].astype(F)
    return out


def stages(grid, size, thres):
    """everything the device stage hands its solve, from the definitions: dict(indices [S, 3], voxel_subvolume [N] (-1 = not eligible), features, weights (of the
    eligible voxels, in list order), gram, weight_sum, A, n, pairs)"""
    keys = np.asarray(grid["keys"]); vs = grid["voxel_size"]; nb = neighbours(grid)
    indices = subvolume_set(keys, vs, size)
    el = eligible(grid, thres, nb)
    vsub = np.full(keys.shape[0], -1, np.int32)
    if size <= 0:
        vsub[el] = 0
    else:
        vsub[el] = _Lookup(indices)(subvolume_index(keys[el], vs, size))
        assert np.all(vsub[el] >= 0)
    f, w = features(grid, el, nb)
    S = indices.shape[0]
    G, ws, A, n = gram(f, w, vsub[el], S)
    return dict(indices=indices, voxel_subvolume=vsub, features=f, weights=w, gram=G, weight_sum=ws, A=A, n=n,
                pairs=pairs(indices) if size > 0 else np.zeros((0, 2), np.int64))


def minimiser(G, ws, prs, lambda_reg):
    """the exact minimiser of the estimate's cost (lighting_svsh.cpp:298-341) by a dense solve: data weight 1 / sum w, regulariser lambda / #pairs on every
    directed pair and coefficient.  Only subvolumes with a data row or a pair carry unknowns; the others keep zeros.  -> ([S, 9], the dense matrix, rhs)"""
    S = G.shape[0]; wsum = math.fsum(ws.tolist()); dw = 1.0 / wsum if wsum > 0 else 1.0
    rw = lambda_reg / len(prs) if len(prs) else 0.0
    H = np.zeros((9 * S, 9 * S)); b = np.zeros(9 * S)
    for s in range(S):
        H[9 * s:9 * s + 9, 9 * s:9 * s + 9] += dw * G[s, :9, :9]; b[9 * s:9 * s + 9] += dw * G[s, :9, 9]
    for i, k in prs:
        for j in range(9):
            a, c = 9 * i + j, 9 * k + j
            H[a, a] += rw; H[c, c] += rw; H[a, c] -= rw; H[c, a] -= rw
    live = np.zeros(S, bool); live[ws > 0] = True
    if len(prs):
        live[np.asarray(prs).ravel()] = True
    u = np.repeat(live, 9)
    x = np.zeros(9 * S)
    if u.any():
        x[u] = np.linalg.lstsq(H[np.ix_(u, u)], b[u], rcond=None)[0]
    return x.reshape(S, 9), H, b
