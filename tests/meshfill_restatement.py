"""The filling of the uncoloured vertices of the mesh colours restated in numpy, written from the definitions (not from
csrc/k_meshfill.hip) on meshstitch_restatement's incidences: the front of means with its levels, the system over the filled vertices, the
Jacobi-preconditioned Chebyshev iteration on [1 / (2 (L + 1))^2, 2] and the bytes.  fp64 throughout; every per-vertex sum is one sequential
addition per incidence in the order of the vertex's corner list, every step the same IEEE operations in the same order as the definition.
The GPU tests hold the kernels to these functions exactly.  exact() is the independent answer: the same system through scipy's spsolve."""
import numpy as np

import meshstitch_restatement as ms

MAX_ITERATIONS = 1000000
UNREACHED = np.iinfo(np.int32).max                           # inside the rounds; -1 in what the functions return


def all_incidences(f, nv):
    """every incidence of every vertex, known or not, in f10's order"""
    return ms.Incidences(f, np.ones(nv, bool))


# ---- the front ----------------------------------------------------------------------------------------------------------------------------
def front(f, rgb, best, max_rounds=0, inc=None):
    """(x float64 [nv, 3], level int32 [nv]: 0 known, 1 .. L reached in that round, -1 unreached; L).  Round r: every vertex of level >= r
    with incidences to vertices of level < r takes the mean of their values -- S = S + x_j in order, S / k -- and the level r.  A round reads
    the levels and values the rounds before it left: a level written in the same round is UNREACHED or r to a reader, never < r."""
    best = np.asarray(best, np.int64).reshape(-1)
    nv = len(best)
    x = np.asarray(rgb, np.uint8).reshape(-1, 3).astype(np.float64)
    level = np.where(best >= 0, 0, UNREACHED).astype(np.int64)
    inc = inc or all_incidences(f, nv)
    I, J = inc.I, inc.J
    r = L = 0
    while not (max_rounds > 0 and r == max_rounds):
        r += 1
        use = (level[I] >= r) & (level[J] < r)
        S = np.zeros((nv, 3), np.float64)
        k = np.zeros(nv, np.int64)
        for m in inc.ranks:
            m = m[use[m]]
            S[I[m]] = S[I[m]] + x[J[m]]
            k[I[m]] += 1
        hit = k > 0
        if not hit.any():
            break
        x[hit] = S[hit] / k[hit].astype(np.float64)[:, None]
        level[hit] = r
        L = r
    return x, np.where(level == UNREACHED, -1, level).astype(np.int32), L


# ---- the system ---------------------------------------------------------------------------------------------------------------------------
def system(f, level, L):
    """(filled bool [nv], Incidences over the known and filled vertices: those of a filled vertex are the system's kept incidences)"""
    level = np.asarray(level, np.int64).reshape(-1)
    filled = (level >= 1) & (level <= L)
    return filled, ms.Incidences(f, filled | (level == 0))


# ---- the solver ---------------------------------------------------------------------------------------------------------------------------
def lmin_of(L):
    w = 2.0 * (float(L) + 1.0)
    return 1.0 / (w * w)


def spectrum(lmin):
    theta, delta = (2.0 + lmin) / 2.0, (2.0 - lmin) / 2.0
    return theta, delta, theta / delta


def auto_steps(L, reduction):
    """the least k >= 1 with T_k(sigma) >= 1 / reduction, the T by f10's recurrence"""
    sigma = spectrum(lmin_of(L))[2]
    target = 1.0 / reduction
    t0, t1, k = 1.0, sigma, 1
    while t1 < target:
        if k == MAX_ITERATIONS:
            raise ValueError("more than %d steps" % MAX_ITERATIONS)
        t0, t1 = t1, (2.0 * sigma) * t1 - t0
        k += 1
    return k


def coefficients(L, steps):
    """[(alpha, beta)] of the steps: f10's recurrence on [lmin_of(L), 2]"""
    theta, delta, sigma = spectrum(lmin_of(L))
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


def solve(f, x, level, L, steps):
    """`steps` steps from x over the filled vertices (1 <= level <= L): S = S + (x_i - x_j) over the kept incidences in order,
    z = (0 - S) / deg (0 for a filled vertex without one: a caller's levels only), d = (alpha d) + (beta z), x' = x + d.  Every other row stays."""
    x = np.array(x, np.float64).reshape(-1, 3)
    filled, inc = system(f, level, L)
    deg = inc.deg.astype(np.float64)[:, None]
    d = np.zeros_like(x)
    for alpha, beta in coefficients(L, steps):
        with np.errstate(all="ignore"):
            z = np.where(deg > 0.0, (0.0 - inc.S(x)) / deg, 0.0)
        d = (alpha * d) + (beta * z)
        x = np.where(filled[:, None], x + d, x)
    return x


def to_bytes(x, rgb, filled):
    """clamp(floor(x + 0.5), 0, 255) for the filled vertices, the input's bytes for the others; and the number of values clamped"""
    q = np.floor(x + 0.5)
    out_of_range = ((q < 0.0) | (q > 255.0)) & filled[:, None]
    out = np.asarray(rgb, np.uint8).reshape(-1, 3).copy()
    out[filled] = np.clip(q, 0.0, 255.0)[filled].astype(np.uint8)
    return out, int(out_of_range.sum())


STAT_KEYS = ("n_vertices", "known", "filled", "unreached", "rounds", "incidences", "dmax", "steps", "clamped", "max_change")


def fill(f, rgb, best, max_rounds=0, iterations=0, reduction=1e-4):
    """the whole call: (rgb uint8 [nv, 3], level int32 [nv], stats dict, x float64 [nv, 3], x_front float64 [nv, 3])"""
    best = np.asarray(best, np.int64).reshape(-1)
    nv = len(best)
    c = np.asarray(rgb, np.uint8).reshape(-1, 3)
    known = int((best >= 0).sum())
    stats = dict({k: 0 for k in STAT_KEYS}, n_vertices=nv, known=known, unreached=nv - known, max_change=0.0)
    x0 = c.astype(np.float64)
    level = np.where(best >= 0, 0, -1).astype(np.int32)
    if known == 0 or known == nv:
        return c.copy(), level, stats, x0, x0
    x0, level, L = front(f, c, best, max_rounds)
    filled, inc = system(f, level, L)
    n = int(filled.sum())
    stats.update(filled=n, unreached=nv - known - n, rounds=L)
    if n == 0:
        return c.copy(), level, stats, x0, x0
    steps = iterations if iterations > 0 else auto_steps(L, reduction)
    x = solve(f, x0, level, L, steps)
    out, clamped = to_bytes(x, c, filled)
    stats.update(incidences=int(inc.deg[filled].sum()), dmax=int(inc.deg[filled].max()), steps=steps, clamped=clamped,
                 max_change=float(np.abs(x - x0)[filled].max()))
    return out, level, stats, x, x0


# ---- an independent answer: the assembled system through a direct solver -----------------------------------------------------------------------
def exact(f, x, level, L):
    """x with the filled rows replaced by the solution of  deg_i x_i - sum over kept incidences to filled j of x_j = sum over those to
    known j of x_j  (scipy's spsolve, per channel)"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    x = np.array(x, np.float64).reshape(-1, 3)
    filled, inc = system(f, level, L)
    idx = np.full(len(filled), -1, np.int64)
    idx[filled] = np.arange(filled.sum())
    n = int(filled.sum())
    own = filled[inc.I]
    I, J = inc.I[own], inc.J[own]
    inner = filled[J]
    A = sp.coo_matrix((np.ones(len(I)), (idx[I], idx[I])), shape=(n, n)) - sp.coo_matrix((np.ones(inner.sum()), (idx[I[inner]], idx[J[inner]])), shape=(n, n))
    b = np.zeros((n, 3))
    np.add.at(b, idx[I[~inner]], x[J[~inner]])
    A = A.tocsc()
    for ch in range(3):
        x[filled, ch] = spsolve(A, b[:, ch])
    return x


def bfs_levels(f, best, max_rounds=0):
    """the breadth-first distance of every vertex from the known ones over the incidence graph, in plain Python: -1 unreached"""
    best = np.asarray(best).reshape(-1)
    nv = len(best)
    adj = [set() for _ in range(nv)]
    for a, b, c in np.asarray(f, np.int64).reshape(-1, 3).tolist():
        if a != b and b != c and a != c:
            adj[a] |= {b, c}
            adj[b] |= {a, c}
            adj[c] |= {a, b}
    level = [0 if best[i] >= 0 else -1 for i in range(nv)]
    cur, r = [i for i in range(nv) if level[i] == 0], 0
    while cur and not (max_rounds > 0 and r == max_rounds):
        r += 1
        nxt = []
        for i in cur:
            for j in adj[i]:
                if level[j] < 0:
                    level[j] = r
                    nxt.append(j)
        cur = nxt
    return np.int32(level)
