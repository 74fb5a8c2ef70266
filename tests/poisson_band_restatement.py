"""numpy restatement of the banded finest level of the Poisson surface (reconstruction_amd/csrc/k_poisson_band.hip).

Test infrastructure only: the package never imports it.  It builds on poisson_restatement.py (f7) by import.  The rules:
  1 samples, grid   f7's steps 1 and 2 at the finest depth D give o and h; the coarse grid has the same o, 2 h and N / 2 nodes per axis
  2 coarse solve    f7's steps 3 to 5 at depth D - 1 on that box -> chi_c (float32)
  3 bricks          B = N / 8 per axis, 8^3 nodes each; occupied = holds a valid sample's (clamped) cell; active = within band_bricks
                    (Chebyshev) of an occupied one; the list ascends in the linear index bx + B (by + B bz); slot = place in the list;
                    fields are brick-major: element slot 512 + lx + 8 (ly + 8 lz)
  4 splat, b        f7's steps 3 and 4 on the active nodes (every node a sample touches is active); occ per fine cell
  5 guess           g = float32(0.25 sum_8 w chi_c): cell-centred trilinear prolongation, per axis 3/4 on the parent and 1/4 on its neighbour
                    towards the fine node, chi_c = 0 outside the coarse grid, summed in fp64 in the corner order dz, dy, dx
  6 band solve      L chi = b on the active nodes; an inactive neighbour holds g, one outside the grid 0.  float32 conjugate gradients from
                    chi = g (the correction e = chi - g from 0), preconditioned by one symmetric red-black Gauss-Seidel sweep from zero on the
                    band (red, black, black, red; colour = (i + j + k) & 1); the residual recomputed from chi every iteration; fp64 dot
                    products; the best iterate kept; ends at rel_residual, max_iterations or STALL iterations without a new best
  7 iso             f7's step 6 on chi
  8 extraction      f7's marching tetrahedra on the cells whose eight corners are active and inside the grid; one vertex per crossed edge
                    (a, direction) with both ends active, in ascending (slot of a, local index of a, direction); faces in (slot, local cell,
                    tetrahedron, triangle) order
  9 trim            f7's step 8 with occ dilated by trim_cells (<= 8 band_bricks - 1, so the dilation stays inside the band)
Dense arrays ([k, j, i], as in f7) carry the band's fields here: the restatement runs at depths where the dense grid is small; to_bricks /
from_bricks change between them and the library's brick-major layout."""
from __future__ import annotations

import numpy as np

import poisson_restatement as pr

STALL = 20         # the library's PB_STALL
MAX_BRICKS = 1 << 20


# ---- 3: bricks --------------------------------------------------------------------------------------------------------------------------
def bricks_of(p, o, h, depth, band_bricks):
    """(occupied bool [B, B, B], active bool [B, B, B], list int32 [S] ascending) from the valid points p"""
    from scipy.ndimage import maximum_filter
    N = 1 << depth
    B = N >> 3
    c = np.clip(np.floor((p - o) / h).astype(np.int64), 0, N - 1) >> 3
    occ = np.zeros((B, B, B), bool)
    occ[c[:, 2], c[:, 1], c[:, 0]] = True
    act = maximum_filter(occ.astype(np.uint8), size=2 * band_bricks + 1, mode="constant", cval=0) != 0
    return occ, act, np.flatnonzero(act.ravel()).astype(np.int32)


def active_of_list(bricks, depth):
    B = (1 << depth) >> 3
    act = np.zeros(B * B * B, bool)
    act[np.asarray(bricks, np.int64)] = True
    return act.reshape(B, B, B)


def node_mask(act):
    """bool [N, N, N]: the node lies in an active brick"""
    return np.repeat(np.repeat(np.repeat(act, 8, 0), 8, 1), 8, 2)


def to_bricks(field, bricks):
    """dense [N, N, N] -> brick-major [S, 512]"""
    N = field.shape[0]
    B = N >> 3
    f = field.reshape(B, 8, B, 8, B, 8).transpose(0, 2, 4, 1, 3, 5).reshape(B * B * B, 512)
    return np.ascontiguousarray(f[np.asarray(bricks, np.int64)])


def from_bricks(values, bricks, depth, fill=0):
    """brick-major [S, 512] -> dense [N, N, N], `fill` off the band"""
    N = 1 << depth
    B = N >> 3
    values = np.asarray(values).reshape(-1, 512)
    f = np.full((B * B * B, 512), fill, values.dtype)
    f[np.asarray(bricks, np.int64)] = values
    return np.ascontiguousarray(f.reshape(B, B, B, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(N, N, N))


# ---- 4: splat and right-hand side ---------------------------------------------------------------------------------------------------------
def band_rhs(xyz, normals, depth, scale=1.1, band_bricks=1):
    """steps 1, 3 and 4: dict p, nh, o, h, b (dense fp64), occ (dense, per fine cell), cnt, occupied, active, bricks, mask"""
    p, nh, ok = pr.valid_samples(xyz, normals)
    o, h = pr.make_grid(p, depth, scale)
    N = 1 << depth
    occb, act, bricks = bricks_of(p, o, h, depth, band_bricks)
    mask = node_mask(act)
    idx, w, inside = pr._trilinear(p, o, h, N)
    q = np.clip(idx, 0, N - 1)
    assert (mask[q[..., 2], q[..., 1], q[..., 0]] | ~inside).all()     # every node a sample touches is active
    V, occ, cnt = pr.splat(p, nh, o, h, depth)
    assert not V[:, ~mask].any() and not occ[~mask].any()
    return dict(p=p, nh=nh, o=o, h=h, b=pr.rhs(V), occ=occ, cnt=cnt, occupied=occb, active=act, bricks=bricks, mask=mask, n_invalid=int((~ok).sum()))


# ---- 5: guess -------------------------------------------------------------------------------------------------------------------------------
def prolong(chi_c):
    """fp64 [N, N, N] from the coarse [N/2, N/2, N/2]: the cell-centred trilinear prolongation at EVERY fine node, 0 outside the coarse grid;
    the eight products are added in the corner order dz, dy, dx"""
    chi_c = np.asarray(chi_c, np.float64)
    Nc = chi_c.shape[0]
    N = 2 * Nc
    P = np.pad(chi_c, 1)                                  # P[x + 1] = chi_c[x], 0 outside
    c = np.arange(N)
    i0 = (c - 1) >> 1                                     # the lower of the two coarse nodes: -1 .. Nc - 1
    f = np.where(c & 1, 0.25, 0.75)                       # the weight of the upper one
    wz, wy, wx = np.meshgrid(f, f, f, indexing="ij")
    acc = np.zeros((N, N, N))
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                w = ((wx if dx else 1.0 - wx) * (wy if dy else 1.0 - wy)) * (wz if dz else 1.0 - wz)
                acc = acc + w * P[np.ix_(i0 + dz + 1, i0 + dy + 1, i0 + dx + 1)]
    return acc


def guess(chi_c32):
    """float32 [N, N, N] from the coarse float32 field: a quarter of its prolongation, rounded once (the solve reads it next to the band too)"""
    return (0.25 * prolong(np.ascontiguousarray(chi_c32, np.float32))).astype(np.float32)


# ---- 6: band solve ----------------------------------------------------------------------------------------------------------------------------
def _band_rbgs(x, b, colour, mask):
    m = pr._colour(x.shape[0], colour) & mask
    x[m] = ((pr._nbr_sum(x) - b) / x.dtype.type(6.0))[m]


def precondition(r, mask):
    """z = M^-1 r: one symmetric red-black Gauss-Seidel sweep from zero on the band, z = 0 off it"""
    z = np.zeros_like(r)
    for colour in (0, 1, 1, 0):
        _band_rbgs(z, r, colour, mask)
    return z


def band_residual(chi, g, b, mask):
    """b - L chi on the band, 0 off it; chi = g at the inactive nodes"""
    r = b - pr._stencil(np.where(mask, chi, g))
    r[~mask] = 0
    return r


def band_pcg(b, g, mask, iterations, dtype=np.float32, stop=0.0, precond=True):
    """The band solve without its best-iterate bookkeeping, in `dtype` with fp64 dot products: (residual before the first iteration, the
    residual after every iteration, the last chi).  b, g dense; b is read on the band only."""
    T = np.dtype(dtype).type
    b = np.where(mask, b, 0).astype(dtype)
    g = np.ascontiguousarray(g, dtype)
    chi = np.where(mask, g, 0).astype(dtype)
    bb = pr._dot64(b, b)
    if not bb > 0.0:
        return 0.0, np.zeros(0), chi
    bnorm = np.sqrt(bb)
    r = band_residual(chi, g, b, mask)
    res0 = np.sqrt(pr._dot64(r, r)) / bnorm
    hist, p, rho_old = [], None, 0.0
    for it in range(1, iterations + 1):
        z = precondition(r, mask) if precond else np.where(mask, -r, 0).astype(dtype)
        rho = pr._dot64(r, z)
        p = z if it == 1 else z + T(rho / rho_old) * p
        q = pr._stencil(p)
        q[~mask] = 0
        pq = pr._dot64(p, q)
        if pq == 0.0 or not np.isfinite(rho / pq):
            break
        chi = chi + T(rho / pq) * p
        r = band_residual(chi, g, b, mask)
        rho_old = rho
        hist.append(np.sqrt(pr._dot64(r, r)) / bnorm)
        if hist[-1] <= stop:
            break
    return float(res0), np.array(hist), chi


def band_solve(b, g, mask, rel_residual, max_iterations, stall=STALL, dtype=np.float32):
    """The band solve as the library ends it: dict chi (the best iterate, dense, g off the band), residual0, residual, iterations, history, status"""
    T = np.dtype(dtype).type
    b = np.where(mask, b, 0).astype(dtype)
    g = np.ascontiguousarray(g, dtype)
    chi = np.where(mask, g, 0).astype(dtype)
    out = dict(chi=np.where(mask, chi, g), residual0=0.0, residual=0.0, iterations=0, history=np.zeros(0), status=0)
    bb = pr._dot64(b, b)
    if not bb > 0.0:
        return out
    bnorm = np.sqrt(bb)
    r = band_residual(chi, g, b, mask)
    best_res = res0 = np.sqrt(pr._dot64(r, r)) / bnorm
    best, hist, p, rho_old, worse, its = chi, [], None, 0.0, 0, 0
    if res0 > rel_residual:
        for it in range(1, max_iterations + 1):
            z = precondition(r, mask)
            rho = pr._dot64(r, z)
            p = z if it == 1 else z + T(rho / rho_old) * p
            q = pr._stencil(p)
            q[~mask] = 0
            pq = pr._dot64(p, q)
            if pq == 0.0 or not np.isfinite(rho / pq):
                break
            chi = chi + T(rho / pq) * p
            r = band_residual(chi, g, b, mask)
            rho_old, its = rho, it
            hist.append(np.sqrt(pr._dot64(r, r)) / bnorm)
            if hist[-1] < best_res:
                best_res, best, worse = hist[-1], chi, 0
                if best_res <= rel_residual:
                    break
            else:
                worse += 1
                if worse >= stall:
                    break
    out.update(chi=np.where(mask, best, g), residual0=float(res0), residual=float(best_res), iterations=its, history=np.array(hist),
               status=0 if best_res <= rel_residual else 1)
    return out


def longest_run_without_best(hist, res0, floor_at=None):
    """the longest run of iterations without a new best residual, up to the iteration of the history's least residual (its floor)"""
    hist = np.asarray(hist)
    end = int(np.argmin(hist)) + 1 if floor_at is None else floor_at
    best, run, longest = res0, 0, 0
    for v in hist[:end]:
        if v < best:
            best, run = v, 0
        else:
            run += 1
            longest = max(longest, run)
    return longest


# ---- 8: extraction ----------------------------------------------------------------------------------------------------------------------------
def _band_ids(bricks, depth):
    """(ident int64 [N^3]: the element slot 512 + local of every node, -1 off the band; nodes int64 [S 512]: the linear node index of every element)"""
    N = 1 << depth
    ident = from_bricks(np.arange(len(bricks) * 512, dtype=np.int64).reshape(-1, 512), bricks, depth, fill=-1).ravel()
    nodes = np.empty(len(bricks) * 512, np.int64)
    on = np.flatnonzero(ident >= 0)
    nodes[ident[on]] = on
    return ident, nodes


def extract_band(chi32, iso, o, h, bricks):
    """chi32 dense float32 (read on the band only) -> (vertices float32 [nv, 3], faces int32 [nf, 3], keys int64 [nv] = 8 (slot 512 + local) +
    direction, dense_keys int64 [nv] = 8 a + direction as f7's extract numbers them)"""
    chi32 = np.ascontiguousarray(chi32, np.float32)
    N = chi32.shape[0]
    depth = int(N).bit_length() - 1
    ident, nodes = _band_ids(bricks, depth)
    iso32 = np.float32(iso)
    flat = chi32.ravel()
    ins = flat < iso32
    ijk = np.stack([nodes % N, (nodes // N) % N, nodes // (N * N)], 1)             # of every element, in element order
    el = np.arange(len(nodes), dtype=np.int64)

    def neighbour(off):
        """(ok, linear node) of element + off: inside the grid and active"""
        q = ijk + np.asarray(off)
        ok = ((q >= 0) & (q < N)).all(1)
        lin = np.where(ok, q[:, 0] + N * (q[:, 1] + N * q[:, 2]), 0)
        return ok & (ident[lin] >= 0), lin

    keys = []
    for d, off in enumerate(pr.DIRS.tolist()):
        ok, lin = neighbour(off)
        cross = ok & (ins[nodes] != ins[lin])
        keys.append(8 * el[cross] + d)
    keys = np.sort(np.concatenate(keys))
    a_el, d = keys // 8, keys % 8
    off = pr.DIRS[d]
    a = nodes[a_el]
    bnode = a + off[:, 0] + N * (off[:, 1] + N * off[:, 2])
    ca, cb = flat[a], flat[bnode]
    t = ((iso32 - ca) / (cb - ca)).astype(np.float32)
    o = np.asarray(o, np.float64)
    pa = (o + (ijk[a_el].astype(np.float64) + 0.5) * h).astype(np.float32)
    pb = (o + ((ijk[a_el] + off).astype(np.float64) + 0.5) * h).astype(np.float32)
    verts = (pa + t[:, None] * (pb - pa)).astype(np.float32)
    dense_keys = 8 * a + d
    # cells: every corner active and inside the grid
    whole = np.ones(len(nodes), bool)
    corner_lin = []
    for c in range(8):
        ok, lin = neighbour((c & 1, (c >> 1) & 1, (c >> 2) & 1))
        whole &= ok
        corner_lin.append(lin)
    cube = np.zeros(len(nodes), np.int64)
    for c in range(8):
        cube |= (ins[corner_lin[c]] & whole).astype(np.int64) << c
    sel_all = np.flatnonzero(whole & (cube != 0) & (cube != 255))
    cases = pr.tet_cases()
    rec = []
    for ti, perm in enumerate(pr.PERMS):
        corner = [0, 1 << perm[0], (1 << perm[0]) | (1 << perm[1]), 7]
        sign = pr.perm_sign(perm)
        m = np.zeros(len(sel_all), np.int64)
        for v in range(4):
            m |= ((cube[sel_all] >> corner[v]) & 1) << v
        for case in range(1, 15):
            sel = sel_all[m == case]
            if len(sel) == 0:
                continue
            for qi, tri in enumerate(cases[case]):
                tri = tri if sign > 0 else (tri[0], tri[2], tri[1])
                ks = []
                for (u, v) in tri:
                    cu, cv = corner[u], corner[v]
                    dd = cv & ~cu
                    na = ident[corner_lin[cu][sel]]
                    ks.append(8 * na + pr.DIR_CODE[(dd & 1, (dd >> 1) & 1, (dd >> 2) & 1)])
                rec.append(np.stack([sel, np.full_like(sel, ti), np.full_like(sel, qi)] + ks, 1))
    if not rec:
        return verts, np.zeros((0, 3), np.int32), keys, dense_keys
    rec = np.concatenate(rec)
    rec = rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))]
    faces = np.searchsorted(keys, rec[:, 3:6]).astype(np.int32)
    assert np.array_equal(keys[faces], rec[:, 3:6])
    return verts, faces, keys, dense_keys


def tet_case_counts_band(chi32, iso, mask):
    """pr.tet_case_counts over the cells whose eight corners are active: int64 [6, 16]"""
    ins = np.ascontiguousarray(chi32, np.float32) < np.float32(iso)
    N = ins.shape[0]
    corner_of = lambda a, c: a[(c >> 2) & 1:, (c >> 1) & 1:, c & 1:][:N - 1, :N - 1, :N - 1]
    whole = np.ones((N - 1,) * 3, bool)
    for c in range(8):
        whole &= corner_of(mask, c)
    out = np.zeros((6, 16), np.int64)
    for ti, perm in enumerate(pr.PERMS):
        corner = [0, 1 << perm[0], (1 << perm[0]) | (1 << perm[1]), 7]
        m = sum(corner_of(ins, corner[v]).astype(np.int64) << v for v in range(4))
        out[ti] = np.bincount(m[whole], minlength=16)
    return out


def trim_band(verts, faces, occ, o, h, trim_cells, band_bricks):
    assert 0 <= trim_cells <= 8 * band_bricks - 1
    return pr.trim(verts, faces, occ, o, h, trim_cells)


# ---- all of it --------------------------------------------------------------------------------------------------------------------------------
def reconstruct_band(xyz, normals, depth, scale=1.1, band_bricks=1, trim_cells=0, rel_residual=4e-5, max_iterations=200, coarse="exact"):
    """Every step.  coarse: 'exact' = the direct fp64 solution of the coarse system rounded to float32, or a float32 array [N/2]^3."""
    R = band_rhs(xyz, normals, depth, scale, band_bricks)
    if isinstance(coarse, str):
        Vc, _, _ = pr.splat(R["p"], R["nh"], R["o"], 2.0 * R["h"], depth - 1)
        coarse = pr.solve_exact(pr.rhs(Vc)).astype(np.float32)
    g = guess(coarse)
    S = band_solve(R["b"], g, R["mask"], rel_residual, max_iterations)
    chi = S["chi"]
    iso = pr.iso_value(chi, R["p"], R["o"], R["h"])
    v0, f0, keys, dkeys = extract_band(chi, iso, R["o"], R["h"], R["bricks"])
    tv, tf = trim_band(v0, f0, R["occ"], R["o"], R["h"], trim_cells, band_bricks)
    R.update(S, g=g, chi_c=coarse, iso=iso, verts0=v0, faces0=f0, keys=keys, dense_keys=dkeys, verts=tv, faces=tf)
    return R


# ---- inputs the tests share ---------------------------------------------------------------------------------------------------------------------
def sparse_fixture():
    """the sphere at scale 3.0, depth 7: the band is a small part of the grid"""
    return pr.sphere_samples(300000), 7, 3.0


def holes_pattern(depth=6):
    """A brick pattern with holes for the extraction: a checkerboard of the bricks ((bx + by + bz) even) plus a solid 3 x 3 x 3 block (bricks
    0..2 per axis); B = 2^(depth - 3) >= 4.  int32 list, ascending."""
    B = (1 << depth) >> 3
    bz, by, bx = np.indices((B, B, B))
    act = ((bx + by + bz) & 1) == 0
    act[:3, :3, :3] = True
    return np.flatnonzero(act.ravel()).astype(np.int32)
