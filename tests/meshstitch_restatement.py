"""The levelling of the views' exposure seams in the mesh colours restated in numpy, written from the definitions (not from
csrc/k_meshstitch.hip) on meshcolor_restatement's pieces: the visibility of every vertex in every view, the incidences of a vertex in the
order of its corner list, the target differences and their sums G, the Jacobi-preconditioned Chebyshev iteration and the bytes.  fp64
throughout; every per-vertex sum is one sequential addition per incidence in the stated order, every step the same IEEE operations in the
same order as the definition (numpy's elementwise operations are IEEE basic operations, never fused).  The GPU tests hold the kernels to
these functions exactly."""
import numpy as np

import meshcolor_restatement as mr

GREY = mr.GREY
MAX_ITERATIONS = 1000000


# ---- what the views see -----------------------------------------------------------------------------------------------------------------
def visibility(v, f, views, min_cos, depth_eps, big_box=4096):
    """f9's visibility test for every (view, vertex), and texture_color's pixel of every vertex in every view:
    (vis bool [V, nv], col float64 [V, nv, 3] red, green, blue)"""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    nv = len(v)
    N = mr.vertex_normals(v, f)
    with np.errstate(all="ignore"):
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        has_n = length > 0.0
        n = N / np.where(has_n, length, 1.0)[:, None]
    p64 = v.astype(np.float64)
    vis = np.zeros((len(views), nv), bool)
    col = np.zeros((len(views), nv, 3), np.float64)
    for k, (P, image, mask) in enumerate(views):
        img = np.asarray(image, np.uint8)
        H, W = img.shape[:2]
        buf = mr.depth_buffer(v, f, P, W, H, False, big_box)
        C = mr.cam_center(P)
        q = mr.project(P, v)
        x, y, inside = mr.pixel_of(q, W, H)
        xi, yi = np.where(inside, x, 0), np.where(inside, y, 0)
        with np.errstate(all="ignore"):
            s = has_n & (q[:, 2] > 0) & inside
            if mask is not None:
                s &= np.asarray(mask, np.uint8)[yi, xi] == 255
            d0, d1, d2 = C[0] - p64[:, 0], C[1] - p64[:, 1], C[2] - p64[:, 2]
            cs = ((n[:, 0] * d0 + n[:, 1] * d1) + n[:, 2] * d2) / np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
            s &= cs > min_cos
            wb = buf[yi, xi]
            s &= (wb == 0) | (q[:, 2].astype(np.float64) <= 1.0 / wb.view(np.float32).astype(np.float64) + depth_eps)
        vis[k] = s
        col[k] = mr.texture_color(v, P, img).astype(np.float64)
    return vis, col


def masks_of(vis):
    """[V, nv] bool -> uint64 [nv], bit v = view v"""
    m = np.zeros(vis.shape[1], np.uint64)
    for k in range(vis.shape[0]):
        m |= vis[k].astype(np.uint64) << np.uint64(k)
    return m


def vis_of(masks, V):
    m = np.asarray(masks, np.uint64)
    return np.stack([((m >> np.uint64(k)) & np.uint64(1)).astype(bool) for k in range(V)]) if V else np.zeros((0, len(m)), bool)


# ---- the incidences ---------------------------------------------------------------------------------------------------------------------
class Incidences:
    """The incidences (i, j) between coloured vertices, sorted by i and within i in the order of its corner list: corners ascending
    3 f + k, per corner f[(k+1)%3] then f[(k+2)%3].  Faces with a repeated index are in no list.  ranks[r] = the positions of every
    vertex's r-th incidence."""

    def __init__(self, f, coloured):
        coloured = np.asarray(coloured, bool)
        self.nv = nv = len(coloured)
        f = np.asarray(f, np.int64).reshape(-1, 3)
        ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]) if len(f) else np.zeros(0, bool)
        fi = np.nonzero(ok)[0]
        own, key, nbr = [], [], []
        for k in range(3):
            for slot, o in enumerate((1, 2)):
                own.append(f[fi, k])
                key.append(2 * (3 * fi + k) + slot)
                nbr.append(f[fi, (k + o) % 3])
        own, key, nbr = (np.concatenate(a) if len(fi) else np.zeros(0, np.int64) for a in (own, key, nbr))
        order = np.lexsort((key, own))
        own, nbr = own[order], nbr[order]
        keep = coloured[own] & coloured[nbr]
        self.I, self.J = own[keep], nbr[keep]
        self.deg = np.bincount(self.I, minlength=nv).astype(np.int64)
        start = np.concatenate([[0], np.cumsum(self.deg)])[:-1]
        rank = np.arange(len(self.I)) - start[self.I]
        self.dmax = int(self.deg.max()) if nv else 0
        self.ranks = [np.nonzero(rank == r)[0] for r in range(self.dmax)]

    def ordered_sum(self, values):
        """out[i] = ((0 + values[first incidence of i]) + values[second]) + ...: one sequential addition per incidence"""
        out = np.zeros((self.nv,) + values.shape[1:], np.float64)
        for m in self.ranks:
            out[self.I[m]] = out[self.I[m]] + values[m]
        return out

    def S(self, x):
        """S_i = sum over i's incidences, in order, of (x_i - x_j)"""
        out = np.zeros_like(x)
        for m in self.ranks:
            i, j = self.I[m], self.J[m]
            out[i] = out[i] + (x[i] - x[j])
        return out


def targets(inc, c, best, vis=None, col=None, seam_gradient=True):
    """the target difference of every incidence, [n, 3], and the counts (incidences, across a seam, with two / one / no term)"""
    I, J = inc.I, inc.J
    a, b = best[I], best[J]
    ci, cj = c[I], c[J]
    seam = a != b
    g = np.where(seam[:, None], 0.0, ci - cj)
    two = one = 0
    if seam_gradient and seam.any():
        a_sees_j = seam & vis[np.where(seam, a, 0), J]
        b_sees_i = seam & vis[np.where(seam, b, 0), I]
        ta = ci - col[np.where(seam, a, 0), J]                # view a's own difference c_i - col_a(j)
        tb = col[np.where(seam, b, 0), I] - cj                # view b's own difference col_b(i) - c_j
        both = a_sees_j & b_sees_i
        g[both] = (ta[both] + tb[both]) / 2.0
        only_a, only_b = a_sees_j & ~b_sees_i, b_sees_i & ~a_sees_j
        g[only_a] = ta[only_a]
        g[only_b] = tb[only_b]
        two, one = int(both.sum()), int(only_a.sum() + only_b.sum())
    n_seam = int(seam.sum())
    counts = dict(incidences=len(I), seam_incidences=n_seam, seam_two_terms=two, seam_one_term=one, seam_no_term=n_seam - two - one)
    return g, counts


def rhs(f, rgb, best, vis=None, col=None, seam_gradient=True):
    """(G float64 [nv, 3], deg int32 [nv], counts) of a colouring"""
    best = np.asarray(best, np.int64)
    inc = Incidences(f, best >= 0)
    g, counts = targets(inc, np.asarray(rgb, np.uint8).astype(np.float64), best, vis, col, seam_gradient)
    return inc.ordered_sum(g), inc.deg.astype(np.int32), counts


# ---- the solver -------------------------------------------------------------------------------------------------------------------------
def spectrum(lam, dmax):
    """(theta, delta, sigma) of the interval [lmin, 2] that holds the eigenvalues of M^-1 A, lmin = lam / (dmax + lam)"""
    lmin = lam / (float(dmax) + lam)
    theta, delta = (2.0 + lmin) / 2.0, (2.0 - lmin) / 2.0
    return theta, delta, theta / delta


def cheb_T(sigma, k):
    """T_0 .. T_k (sigma) by the recurrence T_k+1 = (2 sigma) T_k - T_k-1"""
    t = [1.0, sigma]
    while len(t) <= k:
        t.append((2.0 * sigma) * t[-1] - t[-2])
    return t[:k + 1]


def auto_steps(lam, dmax, reduction):
    """the least k >= 1 with T_k(sigma) >= 1 / reduction, the T by their recurrence"""
    sigma = spectrum(lam, dmax)[2]
    target = 1.0 / reduction
    t0, t1, k = 1.0, sigma, 1
    while t1 < target:
        if k == MAX_ITERATIONS:
            raise ValueError("more than %d steps" % MAX_ITERATIONS)
        t0, t1 = t1, (2.0 * sigma) * t1 - t0
        k += 1
    return k


def coefficients(lam, dmax, steps):
    """[(alpha, beta)] of the steps"""
    theta, delta, sigma = spectrum(lam, dmax)
    rho = 1.0 / sigma
    out = []
    for k in range(steps):
        if k == 0:
            out.append((0.0, 1.0 / theta))
        else:
            rn = 1.0 / (2.0 * sigma - rho)
            out.append((rn * rho, (2.0 * rn) / delta))
            rho = rn
    return out


def solve(f, best, rgb, G, lam, steps, return_inc=False):
    """`steps` steps from x0 = c: (x float64 [nv, 3], the relative residual ||b - A x|| / ||b - A c|| over the coloured vertices).  An
    uncoloured vertex keeps c whatever G holds there."""
    best = np.asarray(best, np.int64)
    col = best >= 0
    inc = Incidences(f, col)
    c = np.asarray(rgb, np.uint8).astype(np.float64).reshape(-1, 3)
    G = np.where(col[:, None], np.asarray(G, np.float64).reshape(-1, 3), 0.0)
    b = G + lam * c
    M = (inc.deg.astype(np.float64) + lam)[:, None]
    x, d = c.copy(), np.zeros_like(c)
    for alpha, beta in coefficients(lam, inc.dmax, steps):
        r = b - (inc.S(x) + lam * x)
        z = r / M
        d = (alpha * d) + (beta * z)
        x = x + d
    r1 = (b - (inc.S(x) + lam * x))[col]
    r0 = (b - (inc.S(c) + lam * c))[col]
    den = np.sqrt((r0 * r0).sum())
    rel = float(np.sqrt((r1 * r1).sum()) / den) if den > 0.0 else 0.0
    return (x, rel, inc) if return_inc else (x, rel)


def to_bytes(x, c, coloured):
    """clamp(floor(x + 0.5), 0, 255) for the coloured vertices, c for the others; and the number of values clamped"""
    q = np.floor(x + 0.5)
    out_of_range = ((q < 0.0) | (q > 255.0)) & coloured[:, None]
    out = np.asarray(c, np.uint8).copy()
    out[coloured] = np.clip(q, 0.0, 255.0)[coloured].astype(np.uint8)
    return out, int(out_of_range.sum())


def stitch(v, f, views, min_cos, depth_eps, lam=0.01, iterations=0, reduction=1e-4, seam_gradient=True, big_box=4096, colouring=None):
    """the whole call: (rgb uint8 [nv, 3], best_view int32 [nv], stats dict, x float64 [nv, 3]).  colouring: (c, best, colour stats, vis, col)
    where a caller has them already (mr.color's mode 0 and visibility() above, same parameters)"""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    nv = len(v)
    c, best, cst = colouring[:3] if colouring else mr.color(v, f, views, 0, min_cos, depth_eps, big_box)
    keys = ("incidences", "seam_incidences", "seam_two_terms", "seam_one_term", "seam_no_term", "dmax", "steps", "clamped")
    stats = dict(n_vertices=nv, coloured=cst["coloured"] if nv else 0, rel_residual=0.0, max_change=0.0, **{k: 0 for k in keys})
    x = c.astype(np.float64)
    if stats["coloured"] == 0:
        return c, best, stats, x
    vis, col = colouring[3:] if colouring else visibility(v, f, views, min_cos, depth_eps, big_box)
    G, deg, counts = rhs(f, c, best, vis, col, seam_gradient)
    dmax = int(deg.max())
    steps = iterations if iterations > 0 else auto_steps(lam, dmax, reduction)
    x, rel = solve(f, best, c, G, lam, steps)
    coloured = best >= 0
    rgb, clamped = to_bytes(x, c, coloured)
    stats.update(counts, dmax=dmax, steps=steps, rel_residual=rel, max_change=float(np.abs(x - c)[coloured].max()), clamped=clamped)
    return rgb, best, stats, x


# ---- an independent answer: the assembled system ------------------------------------------------------------------------------------------
def assemble(inc, lam):
    """A as a scipy CSR matrix over all nv vertices (an uncoloured vertex: the row lam x = ...), and M's diagonal"""
    import scipy.sparse as sp
    n = inc.nv
    A = sp.coo_matrix((np.ones(len(inc.I)), (inc.I, inc.I)), shape=(n, n)) - sp.coo_matrix((np.ones(len(inc.I)), (inc.I, inc.J)), shape=(n, n))
    return (A + lam * sp.identity(n)).tocsc(), inc.deg.astype(np.float64) + lam
