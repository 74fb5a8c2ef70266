"""numpy / scipy restatement of the dense-grid Poisson surface (reconstruction_amd/csrc/k_poisson.hip), fp64.

Test infrastructure only: the package never imports it.  The eight steps:
  1 valid samples   finite point and normal, normal != 0; the normal normalised in fp64
  2 grid            N = 2^depth; lo, hi = bounding box of the valid points; side = scale max(hi - lo); o = (lo + hi) / 2 - side / 2;
                    h = side / N; node (i, j, k) at o + (i + 1/2, j + 1/2, k + 1/2) h; linear index i + N (j + N k)
  3 splat           V(node) = sum w n^ (trilinear, 8 nodes; outside the grid dropped); occ(cell floor((p - o) / h), clamped to the grid) = 1
  4 right-hand side b = 1/2 [(Vx(i+1) - Vx(i-1)) + (Vy(j+1) - Vy(j-1)) + (Vz(k+1) - Vz(k-1))], V = 0 outside
  5 solve           L chi = b, 7-point Laplacian (-6, +1 x 6), chi = 0 outside; scipy's conjugate gradients on -L (solve), the direct
                    solution by sine transforms (solve_exact), and the library's own V-cycle-preconditioned iteration (vcycle, pcg_history)
  6 iso             mean over the valid samples of the trilinear interpolation of chi
  7 extraction      chi < iso is inside; six Kuhn tetrahedra per cell (axis permutations in lexicographic order, path 000 -> +a -> +a+b -> 111);
                    one vertex per crossed lattice edge (a, direction), in ascending (a, direction); faces in (cell, tetrahedron, triangle)
                    order, wound toward growing chi; float32 arithmetic for t and the position, in the kernel's order
  8 trim            occ dilated by trim_cells (Chebyshev); a face survives when the cells floor((v - o) / h) of its three vertices are set
The arrays are indexed [k, j, i] (C order = the linear index)."""
from __future__ import annotations

import itertools

import numpy as np

DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]])   # (x, y, z) of the 7 edge directions
DIR_CODE = {tuple(d): c for c, d in enumerate(DIRS.tolist())}
PERMS = list(itertools.permutations(range(3)))                                                  # lexicographic


def perm_sign(p):
    inv = sum(1 for a in range(len(p)) for b in range(a + 1, len(p)) if p[a] > p[b])
    return -1 if inv & 1 else 1


def tet_cases():
    """The 16 cases of a POSITIVELY oriented tetrahedron (v0..v3; bit i of the case: v_i inside): a list of faces, each three edges
    (u, v), u < v, wound so that the normal points to the outside vertices.  Derived, not copied:
    one vertex L alone, the others A < B < C: (L, A, B, C) is an even permutation iff L is even, and then the face (LA, LB, LC) looks
    away from L; two inside P < Q, two outside R < S: the quad PR, PS, QS, QR looks toward R, S iff (P, Q, R, S) is even."""
    E = lambda u, v: (min(u, v), max(u, v))
    cases = [[] for _ in range(16)]
    for m in range(1, 15):
        ins = [v for v in range(4) if (m >> v) & 1]
        out = [v for v in range(4) if not (m >> v) & 1]
        if len(ins) in (1, 3):
            L = ins[0] if len(ins) == 1 else out[0]
            o = out if len(ins) == 1 else ins
            away = (L & 1) == 0
            want_away = len(ins) == 1
            cases[m] = [(E(L, o[0]), E(L, o[1]), E(L, o[2]))] if away == want_away else [(E(L, o[0]), E(L, o[2]), E(L, o[1]))]
        else:
            P, Q, R, S = ins[0], ins[1], out[0], out[1]
            pr, ps, qs, qr = E(P, R), E(P, S), E(Q, S), E(Q, R)
            cases[m] = [(pr, ps, qs), (pr, qs, qr)] if perm_sign((P, Q, R, S)) > 0 else [(pr, qs, ps), (pr, qr, qs)]
    return cases


def valid_samples(xyz, normals):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    nrm = np.asarray(normals, np.float32).reshape(len(xyz), -1)[:, :3]
    p, n = xyz.astype(np.float64), nrm.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok = np.isfinite(xyz).all(1) & np.isfinite(nrm).all(1) & (nn > 0.0)
    p, n, nn = p[ok], n[ok], nn[ok]
    return p, n / np.sqrt(nn)[:, None], ok


def make_grid(p, depth, scale=1.1):
    """(o [3], h) or None when there is nothing to mesh."""
    if len(p) == 0:
        return None
    lo, hi = p.min(0), p.max(0)
    side = scale * (hi - lo).max()
    if not side > 0.0:
        return None
    o = (lo + hi) / 2.0 - side / 2.0
    return o, side / float(1 << depth)


def _trilinear(p, o, h, N):
    """per sample: node indices [n, 8, 3] (x, y, z), weights [n, 8], inside flags [n, 8]; corner order dz, dy, dx (dx fastest)"""
    g = (p - o) / h - 0.5
    fl = np.floor(g)
    f = g - fl
    i0 = fl.astype(np.int64)
    idx = np.zeros((len(p), 8, 3), np.int64)
    w = np.zeros((len(p), 8))
    c = 0
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                idx[:, c] = i0 + np.array([dx, dy, dz])
                w[:, c] = ((f[:, 0] if dx else 1.0 - f[:, 0]) * (f[:, 1] if dy else 1.0 - f[:, 1])) * (f[:, 2] if dz else 1.0 - f[:, 2])
                c += 1
    ok = ((idx >= 0) & (idx < N)).all(2)
    return idx, w, ok


def splat(p, nh, o, h, depth):
    """V [3, N, N, N] fp64, occ [N, N, N] uint8, cnt [N, N, N] = contributions per node (for the fixed-point bound)"""
    N = 1 << depth
    idx, w, ok = _trilinear(p, o, h, N)
    lin = idx[..., 0] + N * (idx[..., 1] + N * idx[..., 2])
    V = np.zeros((3, N * N * N))
    cnt = np.zeros(N * N * N, np.int64)
    for a in range(3):
        np.add.at(V[a], lin[ok], (w * nh[:, a:a + 1])[ok])
    np.add.at(cnt, lin[ok], 1)
    c = np.clip(np.floor((p - o) / h).astype(np.int64), 0, N - 1)
    occ = np.zeros(N * N * N, np.uint8)
    occ[c[:, 0] + N * (c[:, 1] + N * c[:, 2])] = 1
    return V.reshape(3, N, N, N), occ.reshape(N, N, N), cnt.reshape(N, N, N)


def _shift_diff(A, axis):
    """A(i + 1) - A(i - 1) along `axis`, zero outside"""
    P = np.pad(A, [(1, 1) if a == axis else (0, 0) for a in range(3)])
    sl = lambda s: tuple(s if a == axis else slice(None) for a in range(3))
    return P[sl(slice(2, None))] - P[sl(slice(None, -2))]


def rhs(V):
    # arrays are [k, j, i]: x is axis 2, y axis 1, z axis 0
    return 0.5 * ((_shift_diff(V[0], 2) + _shift_diff(V[1], 1)) + _shift_diff(V[2], 0))


def laplacian(N):
    import scipy.sparse as sp
    d = sp.diags([np.ones(N - 1), -2.0 * np.ones(N), np.ones(N - 1)], [-1, 0, 1], format="csr")
    I = sp.identity(N, format="csr")
    return (sp.kron(sp.kron(d, I), I) + sp.kron(sp.kron(I, d), I) + sp.kron(sp.kron(I, I), d)).tocsr()


def apply_L(chi):
    P = np.pad(chi, 1)
    return (P[1:-1, 1:-1, :-2] + P[1:-1, 1:-1, 2:] + P[1:-1, :-2, 1:-1] + P[1:-1, 2:, 1:-1] + P[:-2, 1:-1, 1:-1] + P[2:, 1:-1, 1:-1]) - 6.0 * chi


def solve(b, rel_residual=1e-10, maxiter=20000):
    """chi [N, N, N] fp64 with ||b - L chi|| / ||b|| <= rel_residual, and the residual reached"""
    import scipy.sparse.linalg as spl
    N = b.shape[0]
    bn = np.linalg.norm(b)
    if bn == 0.0:
        return np.zeros_like(b), 0.0
    A = -laplacian(N)
    x, info = spl.cg(A, -b.ravel(), rtol=rel_residual, atol=0.0, maxiter=maxiter)
    chi = x.reshape(b.shape)
    return chi, float(np.linalg.norm(b - apply_L(chi)) / bn)


def solve_exact(b):
    """The direct solution of L chi = b, independent of any iterative solver: the 7-point Laplacian with chi = 0 outside is diagonal in
    the type-I discrete sine transform, eigenvalues sum over the axes of 2 cos(pi m / (N + 1)) - 2, m = 1..N."""
    from scipy.fft import dstn, idstn
    b = np.asarray(b, np.float64)
    N = b.shape[0]
    lam = 2.0 * np.cos(np.pi * np.arange(1, N + 1) / (N + 1)) - 2.0
    return idstn(dstn(b, type=1) / (lam[:, None, None] + lam[None, :, None] + lam[None, None, :]), type=1)


def laplacian_min_eigenvalue(N):
    """the eigenvalue of -L closest to 0: ||L^-1 r|| <= ||r|| / this"""
    return 3.0 * (2.0 - 2.0 * np.cos(np.pi / (N + 1)))


# ---- step 5 as the library runs it (k_pv_rbgs, k_pv_stencil, k_pv_restrict, k_pv_prolong_add, poisson_solve_device), operation for
# operation in the kernels' order; fields in `dtype`, dot products in fp64 ------------------------------------------------------------
def _nbr_sum(x):
    P = np.pad(x, 1)
    return ((P[1:-1, 1:-1, :-2] + P[1:-1, 1:-1, 2:]) + (P[1:-1, :-2, 1:-1] + P[1:-1, 2:, 1:-1])) + (P[:-2, 1:-1, 1:-1] + P[2:, 1:-1, 1:-1])


def _stencil(x):
    return _nbr_sum(x) - x.dtype.type(6.0) * x


_colour_masks = {}


def _colour(n, colour):
    if (n, colour) not in _colour_masks:
        k, j, i = np.indices((n, n, n))
        _colour_masks[n, colour] = ((i + j + k) & 1) == colour
    return _colour_masks[n, colour]


def _rbgs(x, b, colour):
    m = _colour(x.shape[0], colour)
    x[m] = ((_nbr_sum(x) - b) / x.dtype.type(6.0))[m]


def vcycle(b, dtype=np.float64):
    """x = M^-1 b: one V-cycle from x = 0.  Red-black Gauss-Seidel (red, black) down, the residual, coarse right-hand side = 0.5 x the
    sum of the 8 residuals of a coarse cell (= 4 x their mean: the same stencil at 2h), the coarse cycle, piecewise-constant
    prolongation added, Gauss-Seidel (black, red) up; at 2^3 eight sweeps (red, black) and eight (black, red)."""
    b = np.ascontiguousarray(b, dtype)
    n = b.shape[0]
    x = np.zeros_like(b)
    if n == 2:
        for s in range(16):
            for c in range(2):
                _rbgs(x, b, c if s < 8 else 1 - c)
        return x
    for c in range(2):
        _rbgs(x, b, c)
    r = b - _stencil(x)
    s = (((r[0::2, 0::2, 0::2] + r[0::2, 0::2, 1::2]) + (r[0::2, 1::2, 0::2] + r[0::2, 1::2, 1::2]))
         + ((r[1::2, 0::2, 0::2] + r[1::2, 0::2, 1::2]) + (r[1::2, 1::2, 0::2] + r[1::2, 1::2, 1::2])))
    xc = vcycle(b.dtype.type(0.5) * s, dtype)
    x += np.repeat(np.repeat(np.repeat(xc, 2, 0), 2, 1), 2, 2)
    for c in range(2):
        _rbgs(x, b, 1 - c)
    return x


def _dot64(x, y):
    return float(np.dot(x.ravel().astype(np.float64), y.ravel().astype(np.float64)))


def pcg_history(b, cycles, dtype=np.float64, stop=0.0):
    """Conjugate gradients preconditioned by vcycle, as poisson_solve_device runs them without its best-iterate bookkeeping: chi from 0,
    the residual recomputed from chi every cycle, fp64 dot products, the two step lengths rounded to `dtype`.  Returns (the relative
    residual after every cycle, the last chi); ends after `cycles` cycles or at the first residual <= stop."""
    b = np.ascontiguousarray(b, dtype)
    T = b.dtype.type
    chi = np.zeros_like(b)
    hist = []
    bb = _dot64(b, b)
    if not bb > 0.0:
        return np.zeros(0), chi
    bnorm = np.sqrt(bb)
    r, p, rho_old = b.copy(), None, 0.0
    for it in range(1, cycles + 1):
        z = vcycle(r, dtype)
        rho = _dot64(r, z)
        p = z if it == 1 else z + T(rho / rho_old) * p
        q = _stencil(p)
        pq = _dot64(p, q)
        if pq == 0.0 or not np.isfinite(rho / pq):
            break
        chi = chi + T(rho / pq) * p
        r = b - _stencil(chi)
        rho_old = rho
        hist.append(np.sqrt(_dot64(r, r)) / bnorm)
        if hist[-1] <= stop:
            break
    return np.array(hist), chi


def iso_value(chi, p, o, h):
    N = chi.shape[0]
    idx, w, ok = _trilinear(p, o, h, N)
    idx = np.clip(idx, 0, N - 1)
    val = np.where(ok, w * chi.astype(np.float64)[idx[..., 2], idx[..., 1], idx[..., 0]], 0.0)
    return float(val.sum(1).sum() / len(p))


def extract(chi32, iso, o, h):
    """chi32 [N, N, N] float32 -> (vertices float32 [nv, 3], faces int32 [nf, 3], keys int64 [nv] = 8 a + direction)"""
    chi32 = np.ascontiguousarray(chi32, np.float32)
    N = chi32.shape[0]
    iso32 = np.float32(iso)
    ins = (chi32 < iso32).ravel()
    flat = chi32.ravel()
    lin = np.arange(N * N * N, dtype=np.int64)
    ijk = np.stack([lin % N, (lin // N) % N, lin // (N * N)], 1)
    # vertices: crossed edges in ascending (a, direction)
    keys = []
    for d, (dx, dy, dz) in enumerate(DIRS.tolist()):
        okb = (ijk[:, 0] + dx < N) & (ijk[:, 1] + dy < N) & (ijk[:, 2] + dz < N)
        a = lin[okb]
        b = a + dx + N * (dy + N * dz)
        cross = ins[a] != ins[b]
        keys.append(8 * a[cross] + d)
    keys = np.sort(np.concatenate(keys))
    a, d = keys // 8, keys % 8
    off = DIRS[d]
    b = a + off[:, 0] + N * (off[:, 1] + N * off[:, 2])
    ca, cb = flat[a], flat[b]
    t = ((iso32 - ca) / (cb - ca)).astype(np.float32)
    o = np.asarray(o, np.float64)
    pa = (o + (ijk[a].astype(np.float64) + 0.5) * h).astype(np.float32)
    pb = (o + ((ijk[a] + off).astype(np.float64) + 0.5) * h).astype(np.float32)
    verts = (pa + t[:, None] * (pb - pa)).astype(np.float32)
    # faces: per (cell, tetrahedron, triangle)
    cases = tet_cases()
    cell_ok = (ijk[:, 0] < N - 1) & (ijk[:, 1] < N - 1) & (ijk[:, 2] < N - 1)
    cells = lin[cell_ok]
    st = np.array([1, N, N * N], np.int64)
    cube = np.zeros(len(cells), np.int64)
    for c in range(8):
        cube |= ins[cells + (c & 1) * st[0] + ((c >> 1) & 1) * st[1] + ((c >> 2) & 1) * st[2]].astype(np.int64) << c
    act = (cube != 0) & (cube != 255)
    cells, cube = cells[act], cube[act]
    rec = []   # (cell, tet, tri, key0, key1, key2)
    for ti, perm in enumerate(PERMS):
        corner = [0, 1 << perm[0], (1 << perm[0]) | (1 << perm[1]), 7]
        sign = perm_sign(perm)
        m = np.zeros(len(cells), np.int64)
        for v in range(4):
            m |= ((cube >> corner[v]) & 1) << v
        for case in range(1, 15):
            sel = cells[m == case]
            if len(sel) == 0:
                continue
            for qi, tri in enumerate(cases[case]):
                tri = tri if sign > 0 else (tri[0], tri[2], tri[1])
                ks = []
                for (u, v) in tri:
                    cu, cv = corner[u], corner[v]
                    dd = cv & ~cu
                    na = sel + (cu & 1) * st[0] + ((cu >> 1) & 1) * st[1] + ((cu >> 2) & 1) * st[2]
                    ks.append(8 * na + DIR_CODE[(dd & 1, (dd >> 1) & 1, (dd >> 2) & 1)])
                rec.append(np.stack([sel, np.full_like(sel, ti), np.full_like(sel, qi)] + ks, 1))
    if not rec:
        return verts, np.zeros((0, 3), np.int32), keys
    rec = np.concatenate(rec)
    rec = rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))]
    faces = np.searchsorted(keys, rec[:, 3:6]).astype(np.int32)
    assert np.array_equal(keys[faces], rec[:, 3:6])
    return verts, faces, keys


def vertex_cells(verts, o, h, N):
    c = np.floor((np.asarray(verts, np.float32).astype(np.float64) - np.asarray(o, np.float64)) / h).astype(np.int64)
    return np.clip(c, 0, N - 1)


def dilate(occ, trim_cells):
    from scipy.ndimage import maximum_filter
    return maximum_filter(occ, size=2 * trim_cells + 1, mode="constant", cval=0)


def trim(verts, faces, occ, o, h, trim_cells):
    if trim_cells <= 0:
        return verts, faces
    N = occ.shape[0]
    c = vertex_cells(verts, o, h, N)
    vk = dilate(occ, trim_cells)[c[:, 2], c[:, 1], c[:, 0]] != 0
    keep = vk[faces].all(1) & (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    f = faces[keep]
    used = np.zeros(len(verts), bool)
    used[f.ravel()] = True
    new = np.cumsum(used) - 1
    return verts[used], new[f].astype(np.int32)


def reconstruct(xyz, normals, depth, scale=1.1, rel_residual=1e-10, trim_cells=0):
    """All eight steps.  Returns a dict: verts, faces, chi (fp64), chi32, iso, o, h, occ, b, cnt, residual (or verts / faces empty)."""
    p, nh, ok = valid_samples(xyz, normals)
    g = make_grid(p, depth, scale)
    if g is None:
        return dict(verts=np.zeros((0, 3), np.float32), faces=np.zeros((0, 3), np.int32), o=None, h=0.0)
    o, h = g
    V, occ, cnt = splat(p, nh, o, h, depth)
    b = rhs(V)
    chi, res = solve(b, rel_residual)
    iso = iso_value(chi, p, o, h)
    chi32 = chi.astype(np.float32)
    verts, faces, keys = extract(chi32, iso, o, h)
    tv, tf = trim(verts, faces, occ, o, h, trim_cells)
    return dict(verts=tv, faces=tf, verts0=verts, faces0=faces, keys=keys, chi=chi, chi32=chi32, iso=iso, o=o, h=h, occ=occ, b=b, cnt=cnt,
                residual=res, p=p, nh=nh)


# ---- inputs and checks the tests share -----------------------------------------------------------------------------------------------
SPHERE_C = np.array([10.0, -20.0, 600.0])
SPHERE_R = 50.0


def sphere_samples(n, seed=1, noise=0.05, cap=False):
    """n noisy samples of the sphere (radius 50 around (10, -20, 600)) with outward normals; cap: only those with n^z < -0.3"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = SPHERE_R + noise * rng.normal(size=n)
    xyz = (SPHERE_C + d * r[:, None]).astype(np.float32)
    nrm = np.zeros((n, 4), np.float32)
    nrm[:, :3] = d
    if cap:
        keep = d[:, 2] < -0.3
        xyz, nrm = xyz[keep], nrm[keep]
    return xyz, nrm


def _with_normals(xyz, d):
    nrm = np.zeros((len(xyz), 4), np.float32)
    nrm[:, :3] = d
    return np.asarray(xyz, np.float32), nrm


TORUS_C = np.array([-300.0, 7.0, -2.5])
TORUS_R, TORUS_r = 40.0, 15.0


def torus_samples(n, seed=2, noise=0.05):
    """Of n draws, those an area-uniform rejection keeps (about 3/4): noisy samples of the torus around TORUS_C (axis z, R = 40, r = 15)
    with outward normals.  Away from the sphere's coordinates: x near -300, y and z on both sides of 0."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(0.0, 2.0 * np.pi, n)
    keep = rng.uniform(size=n) * (TORUS_R + TORUS_r) <= TORUS_R + TORUS_r * np.cos(v)
    rr = TORUS_r + noise * rng.normal(size=n)
    u, v, rr = u[keep], v[keep], rr[keep]
    d = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    ring = np.stack([TORUS_R * np.cos(u), TORUS_R * np.sin(u), np.zeros_like(u)], 1)
    return _with_normals(TORUS_C + ring + d * rr[:, None], d)


def torus_distance(verts):
    q = np.asarray(verts, np.float64) - TORUS_C
    return np.abs(np.hypot(np.hypot(q[:, 0], q[:, 1]) - TORUS_R, q[:, 2]) - TORUS_r)


TWO_C = np.array([[-20.0, 3.0, -1.0], [-20.0 + 33.6, 3.0 + 44.8, -1.0]])      # 56 apart
TWO_R = np.array([30.0, 12.0])


def two_spheres_samples(n, seed=3, noise=0.05):
    """n noisy samples of two spheres (radii 30 and 12, centres 56 apart: a gap of 14), shared by area, outward normals"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    which = (rng.uniform(size=n) * (TWO_R ** 2).sum() >= TWO_R[0] ** 2).astype(np.int64)
    r = TWO_R[which] + noise * rng.normal(size=n)
    return _with_normals(TWO_C[which] + d * r[:, None], d)


def two_spheres_distance(verts):
    v = np.asarray(verts, np.float64)
    return np.abs(np.linalg.norm(v[:, None, :] - TWO_C[None], axis=2) - TWO_R).min(1)


PLATE_LO, PLATE_HI, PLATE_Z = np.array([-96.0, -40.0]), np.array([32.0, 40.0]), -7.5


def plate_samples(n, seed=4):
    """n samples of the rectangle [-96, 32] x [-40, 40] at z = -7.5 (zero extent along z), normals +z; the first four are its corners,
    so at scale = 1.0 (side 128, h = 128 / N, all exact in binary) samples lie on the grid box's faces x = o and x = o + N h."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(PLATE_LO, PLATE_HI, size=(n, 2))
    xy[:4] = [[PLATE_LO[0], PLATE_LO[1]], [PLATE_HI[0], PLATE_LO[1]], [PLATE_LO[0], PLATE_HI[1]], [PLATE_HI[0], PLATE_HI[1]]]
    xyz = np.concatenate([xy, np.full((n, 1), PLATE_Z)], 1)
    return _with_normals(xyz, np.tile([0.0, 0.0, 1.0], (n, 1)))


def rhs_of(xyz, normals, depth, scale=1.1):
    """steps 1 to 4 alone: dict p, nh, o, h, b, occ, cnt"""
    p, nh, ok = valid_samples(xyz, normals)
    o, h = make_grid(p, depth, scale)
    V, occ, cnt = splat(p, nh, o, h, depth)
    return dict(p=p, nh=nh, o=o, h=h, b=rhs(V), occ=occ, cnt=cnt)


def rhs_fixed_point_bound(cnt, b_ref):
    """The bound on |b - b_ref| of a splat that adds llrint(w n^ 2^32): each contribution is off by at most half a unit, 2^-33.  A node's V is
    off by cnt(node) 2^-33 (cnt = contributions, counted by the restatement), and b = 1/2 (six neighbour values) by 1/2 sum_6 cnt(neighbour)
    2^-33; the integer differences and their conversion are exact.  The restatement's own fp64 sums round by at most cnt^2 2^-53 per node
    (partial sums <= cnt), and its three additions and the product by 2^-50 (1 + |b|)."""
    cnt = np.asarray(cnt, np.float64)

    def six(a):
        p = np.pad(a, 1)
        return p[1:-1, 1:-1, :-2] + p[1:-1, 1:-1, 2:] + p[1:-1, :-2, 1:-1] + p[1:-1, 2:, 1:-1] + p[:-2, 1:-1, 1:-1] + p[2:, 1:-1, 1:-1]
    return 0.5 * six(cnt) * 2.0 ** -33 + 0.5 * six(cnt * cnt) * 2.0 ** -53 + 2.0 ** -50 * (1.0 + np.abs(b_ref))


def node_centre_samples(N=32):
    """Samples exactly on node centres of the grid they define at scale = 1.0 (all but one trilinear weight 0): the nodes of a 2^5 lattice of
    spacing 2 nearest a sphere of radius 20, at odd offsets from (-200, 0, 100), and two samples that pin the bounding box to 64 a side."""
    k, j, i = np.indices((N, N, N))
    q = np.stack([i, j, k], -1).reshape(-1, 3) * 2.0 + 1.0
    d = q - np.array([33.0, 31.0, 35.0])
    r = np.linalg.norm(d, axis=1)
    sel = np.abs(r - 20.0) <= 1.0
    lo = np.array([-200.0, 0.0, 100.0])
    xyz = np.concatenate([[lo, lo + 2.0 * N], lo + q[sel]])
    nrm = np.concatenate([[[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], d[sel] / r[sel, None]])
    return _with_normals(xyz, nrm)


def solver_rhs(kind, depth=5):
    """The right-hand sides the solver is held to: 'sphere' = the noisy sphere's; 'random' = seeded normal values (every frequency);
    'corners' = zero but for the nodes (0, 0, 0), (N-1, N-1, N-1) and one on an edge of the box (the boundary terms of every kernel)."""
    N = 1 << depth
    if kind == "sphere":
        return rhs_of(*sphere_samples(20000 * 4 ** (depth - 5)), depth)["b"]
    if kind == "random":
        return np.random.default_rng(21).normal(size=(N, N, N))
    b = np.zeros((N, N, N))
    b[0, 0, 0], b[N - 1, N - 1, N - 1], b[0, N - 1, N // 3] = 1.0, -0.75, 0.5
    return b


FIELD_O, FIELD_H = np.array([-3.5, 7.25, 100.0]), 0.37


def lattice_field(kind, N=32):
    """Constructed fields for the extraction, (chi float32 [N, N, N], iso): 'random' = seeded normal values, the surface runs into every
    face of the lattice and every tetrahedron case occurs; 'closed' = the same with the outermost node layer forced outside;
    'tie0' / 'tie1' = integers -2..2 with iso 0 / 1 one of them (t = 0, coincident vertices, zero-area faces)."""
    if kind in ("random", "closed"):
        chi = np.random.default_rng(11).normal(size=(N, N, N)).astype(np.float32)
        iso = 0.1
        assert not (chi == np.float32(iso)).any()
        if kind == "closed":
            chi[[0, -1]] = chi[:, [0, -1]] = chi[:, :, [0, -1]] = 5.0
        return chi, iso
    chi = np.random.default_rng(12).integers(-2, 3, size=(N, N, N)).astype(np.float32)
    return chi, {"tie0": 0.0, "tie1": 1.0}[kind]


def edge_ends(keys, N):
    """the two lattice nodes (x, y, z) of each emitted vertex, from extract's keys = 8 a + direction: (int64 [nv, 3], int64 [nv, 3])"""
    keys = np.asarray(keys, np.int64)
    a, d = keys // 8, keys % 8
    na = np.stack([a % N, (a // N) % N, a // (N * N)], 1)
    return na, na + DIRS[d]


def _undirected_edges(faces, nv):
    """(int64 [ne, 2] the distinct undirected edges, the number of faces on each)"""
    f = np.asarray(faces, np.int64)
    und = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    uk, cnt = np.unique(und[:, 0] * np.int64(nv + 1) + und[:, 1], return_counts=True)     # int64: nv (nv + 1) passes 2^31
    return np.stack([uk // (nv + 1), uk % (nv + 1)], 1), cnt


def boundary_edge_report(verts, faces, keys, N):
    """The open-border rule of the extraction.  A mesh edge lies in one of the six boundary planes of the node lattice (a coordinate 0 or
    N - 1) when both its vertices sit on lattice edges whose two nodes are in that plane; such an edge belongs to one tetrahedron
    face that no second cell shares, and is in one face; every other edge is in two.  Counts by faces per edge and by in / off plane."""
    na, nb = edge_ends(keys, N)
    bits = np.zeros(len(keys), np.int64)
    for c in range(3):
        for s, val in enumerate((0, N - 1)):
            bits |= ((na[:, c] == val) & (nb[:, c] == val)).astype(np.int64) << (2 * c + s)
    e, cnt = _undirected_edges(faces, len(verts))
    inp = (bits[e[:, 0]] & bits[e[:, 1]]) != 0
    return dict(once_in_plane=int(((cnt == 1) & inp).sum()), once_off_plane=int(((cnt == 1) & ~inp).sum()),
                twice_in_plane=int(((cnt == 2) & inp).sum()), twice_off_plane=int(((cnt == 2) & ~inp).sum()),
                more_than_twice=int((cnt > 2).sum()))


def orientation_products(verts, faces, keys, chi32, iso, o, h):
    """per face: normal . (mean of its three vertices' outside nodes - mean of their inside nodes); > 0 = wound toward growing chi"""
    chi32 = np.ascontiguousarray(chi32, np.float32)
    N = chi32.shape[0]
    na, nb = edge_ends(keys, N)
    a_in = chi32[na[:, 2], na[:, 1], na[:, 0]] < np.float32(iso)
    b_in = chi32[nb[:, 2], nb[:, 1], nb[:, 0]] < np.float32(iso)
    assert (a_in != b_in).all()
    pos = lambda ijk: np.asarray(o, np.float64) + (ijk + 0.5) * h
    inside, outside = pos(np.where(a_in[:, None], na, nb)), pos(np.where(a_in[:, None], nb, na))
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return np.einsum("ij,ij->i", n, outside[f].mean(1) - inside[f].mean(1))


def tet_case_counts(chi32, iso):
    """int64 [6, 16]: how many cells put tetrahedron t (PERMS order) into case m (bit v: corner v inside)"""
    ins = np.ascontiguousarray(chi32, np.float32) < np.float32(iso)
    out = np.zeros((6, 16), np.int64)
    corner_of = lambda c: ins[(c >> 2) & 1:, (c >> 1) & 1:, c & 1:][:ins.shape[0] - 1, :ins.shape[1] - 1, :ins.shape[2] - 1]
    for ti, perm in enumerate(PERMS):
        corner = [0, 1 << perm[0], (1 << perm[0]) | (1 << perm[1]), 7]
        m = sum(corner_of(corner[v]).astype(np.int64) << v for v in range(4))
        out[ti] = np.bincount(m.ravel(), minlength=16)
    return out


def components(faces, nv):
    """the number of edge-connected components of the faces"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64)
    he = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    owner = np.tile(np.arange(len(f)), 3)
    und = np.sort(he, 1)
    key = und[:, 0] * np.int64(nv + 1) + und[:, 1]
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    g = sp.coo_matrix((np.ones(same.sum()), (owner[order][1:][same], owner[order][:-1][same])), shape=(len(f), len(f)))
    return int(connected_components(g, directed=False)[0])


def manifold_report(verts, faces):
    """The exact conditions of a closed oriented 2-manifold: dict of counts that must all be as stated in the tests."""
    f = np.asarray(faces, np.int64)
    nv = len(verts)
    rep = dict(index_out_of_range=int(((f < 0) | (f >= nv)).sum()),
               repeated_index=int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum()))
    he = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    dk = he[:, 0] * (nv + 1) + he[:, 1]
    rep["directed_edge_twice"] = int(len(dk) - len(np.unique(dk)))
    rk = he[:, 1] * (nv + 1) + he[:, 0]
    rep["edge_without_opposite"] = int((~np.isin(dk, rk)).sum())
    und = np.sort(he, 1)
    uk, cnt = np.unique(und[:, 0] * (nv + 1) + und[:, 1], return_counts=True)
    rep["edges_not_in_two_faces"] = int((cnt != 2).sum())
    rep["euler"] = int(nv - len(uk) + len(f))
    rep["unused_vertices"] = int(nv - len(np.unique(f)))
    return rep


def radial_error_h(verts, h):
    return np.abs(np.linalg.norm(np.asarray(verts, np.float64) - SPHERE_C, axis=1) - SPHERE_R) / h


def face_orientation_min(verts, faces):
    """min over the faces of (geometric normal) . (radial direction at the centroid), both unnormalised"""
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = np.cross(b - a, c - a)
    return float(np.einsum("ij,ij->i", n, (a + b + c) / 3.0 - SPHERE_C).min())


def read_ply_mesh(path):
    """A small reader of rsm_write_ply_mesh's files: (vertices float32 [nv, 3], faces int32 [nf, 3])"""
    with open(path, "rb") as fp:
        assert fp.readline() == b"ply\n"
        assert fp.readline() == b"format binary_little_endian 1.0\n"
        nv = nf = None
        props = []
        while True:
            line = fp.readline().decode().strip()
            if line == "end_header":
                break
            if line.startswith("element vertex"):
                nv = int(line.split()[2])
            elif line.startswith("element face"):
                nf = int(line.split()[2])
            elif line.startswith("property"):
                props.append(line)
        assert props == ["property float x", "property float y", "property float z", "property list uchar int vertex_indices"], props
        v = np.frombuffer(fp.read(12 * nv), "<f4").reshape(nv, 3)
        rec = np.frombuffer(fp.read(13 * nf), np.dtype([("n", "u1"), ("i", "<i4", 3)]))
        assert fp.read() == b""
        assert (rec["n"] == 3).all()
        return v.copy(), rec["i"].astype(np.int32).reshape(nf, 3)
