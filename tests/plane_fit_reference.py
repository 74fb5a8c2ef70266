"""An eigen-solver and a least-squares solver that share no formula with the cloud kernels' local plane fit (pcl_plane_from_cov in
csrc/cloud_grid.h, behind k_cloud_normals, k_normals_lattice and k_mls<0|1|2>), the bounds the kernels are held to against them, the
census of the branches a neighbourhood takes, and the lattice fixture that reaches the rare ones.  numpy only; test infrastructure.

  neighbourhoods   brute force, the kernels' membership rule: finite q with float32 (dx*dx + dy*dy) + dz*dz < fl32(r*r), p included.
  plane            two-pass covariance in numpy.longdouble, numpy.linalg.eigh: normal = the eigenvector of the smallest eigenvalue l0,
                   curvature l0 / trace, conditioning kappa = l2 / (l1 - l0) and, for the one-pass kernels (covariance E[xx^T] - cc^T),
                   kappa1 = (l2 + cnt |c|^2) / (l1 - l0).  The sign is not the solver's business: compare up to sign and check the
                   orientation rule on its own.
  fit              orders 1 and 2: the restatement's frame and terms, solved by numpy.linalg.lstsq on sqrt(w) P, sqrt(w) f (an SVD, not
                   the normal equations); the projected point, the unnormalised normal, the 2-norm condition number of P W P^T.
  census           mls_restatement.plane_from_cov / mls, instrumented: root path, cross-product pick and ties, unitOrthogonal's form,
                   cnt against NC, the Cholesky pivots, c[0] finite.
  lattice_fixture  clusters on an exact lattice (coordinates multiples of 0.25, origins multiples of 16 up to 1024, diameter below
                   r = 2.5, more than 3 r apart): every sum is exact in double, which exact_two_pass / exact_one_pass check with
                   fractions.Fraction, so neither the order of summation nor a fused multiply-add can change a result or a
                   branch where that is claimed.

Bounds.  With u = 2^-24 (a float32 normal component's rounding; ulp32(x) / 2 for a coordinate or a curvature) and e = 2^-52:
  normals, order 0        u (1 + d) + K e kappa             (kappa1 for the one-pass kernels)
  curvature               ulp32 / 2 (1 + d) + K e l2 / trace   ((l2 + cnt |c|^2) / trace for the one-pass kernels)
  MLS positions           ulp32 / 2 (1 + d) + K e ((kappa + cond(P W P^T)) r + |x|)     (cond = 0 where no polynomial is fitted;
                          |x|: the coordinate's own rounding in double)
  MLS normals, order > 0  max(1, |n_i|) u (1 + d) + K e (kappa + cond(P W P^T))
(K, d) per line are the worst figures of the CPU references (mls_restatement orders 0 / 1 / 2, oracle.cloud_normals) against these
solvers over the lattice fixture, surface_cloud(6000, 2) at r = 2.5 and surface_cloud(3000, 3) at r = 1.2, measured by
tests/test_plane_fit_cpu.py -- d on the points whose conditioning term is below 2^-12 of the rounding term, K on all -- and on
"sheet", a crop of the thin-sheet test pair's cloud at the pixel-lattice route's radius 9 (neighbourhoods of ~300 points at |c| ~ 1700:
the nine sums' accumulated rounding, which neighbourhoods of 50 points do not show), and stated in MEASURED below
(rounded up, and never below 1: no backward-stable eigenvector or solve does better than e times its conditioning); that test fails
if the references exceed them.  The kernels get 4 K: their exp, atan2, cos and sin are other
implementations of the same last-bit quality and fused multiply-add reorders roundings.  A point whose l1 - l0 is within 4 e l2 (the
eigen-solver's own rounding: no eigenvector to compare with) is left out and counted.
Measured K (stated): normals two-pass 0 (1), one-pass 0.17 (1); curvature two-pass 208.8 (210: the cubic's roots lose digits where l0
and l1 are close), one-pass 9.12 (9.5: a rounding per neighbour in the nine sums, 300 neighbours); positions 5e-20 (1); fitted normals
4e-19 (1).  Measured d: 0 for every line -- away from ill conditioning the references' errors are the float32 rounding itself.

The restated PCL has no plane for some neighbourhoods of 3 points and more -- a line, a repeated point (every cross product of
eigen33 is 0: 0 / 0), an isotropic covariance (cube corners: NaN normal, curvature 1 / 3) -- and MLS then emits a NaN point.  That is
PCL 1.7.2's behaviour; it is pinned here as it is.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from mls_restatement import _cross, _terms, plane_from_cov, unit_orthogonal

U32 = 2.0 ** -24
E64 = 2.0 ** -52
R_LATTICE = 2.5

# (K, d) per bound: see the docstring.  Measured values in profiles/f25_plane_fit_tests.log.
MEASURED = {
    "normal2": (1.0, 0.0),       # measured K 0 (every error is float32 rounding, 2^-25): the floor of 1 stands
    "normal1": (1.0, 0.0),       # measured K 0.17
    "curv2": (210.0, 0.0),       # measured K 208.8 (sparse): the cubic's roots lose digits where l0 and l1 are close (kappa 3e3 there)
    "curv1": (9.5, 0.0),         # measured K 9.12 (sheet: 300 roundings in each of the nine sums); 1.22 on the other fixtures
    "pos": (1.0, 0.0),           # measured K 5e-20
    "fitnormal": (1.0, 0.0),     # measured K 4e-19
}
KERNEL_K = 4.0


def half_ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64) / 2.0


def measure(err, rnd, cond):
    """(K, d) of err <= rnd (1 + d) + K cond over the given points: d where cond < rnd / 4096 (nothing but the float32 rounding can
    show there), then K on all."""
    err, rnd, cond = (np.asarray(a, np.float64).ravel() for a in np.broadcast_arrays(err, rnd, cond))
    ok = np.isfinite(err) & np.isfinite(cond)
    err, rnd, cond = err[ok], rnd[ok], cond[ok]
    small = cond < rnd / 4096.0
    with np.errstate(all="ignore"):
        d = max(0.0, float(np.max(err[small] / rnd[small] - 1.0, initial=0.0)))
        over = err - rnd * (1.0 + d)
        K = float(np.max(np.where((over > 0.0) & (cond > 0.0), over / cond, 0.0), initial=0.0))
    return K, d


def bound(rnd, cond, which, mult=1.0):
    K, d = MEASURED[which]
    return rnd * (1.0 + d) + mult * K * cond


# ---------------------------------------------------------------- neighbourhoods
def neighbourhoods(xyz, r, queries=None, block=512):
    """CSR (ptr [q + 1], idx) of the radius neighbourhoods of the queried points (default: all) among all points of xyz."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    q_idx = np.arange(len(xyz)) if queries is None else np.asarray(queries, np.int64).ravel()
    fin = np.isfinite(xyz).all(1)
    cand = np.nonzero(fin)[0]
    X = xyz[cand]
    r2f = np.float32(float(r) * float(r))
    cnt = np.zeros(len(q_idx), np.int64)
    cols = []
    for b0 in range(0, len(q_idx), block):
        Q = xyz[q_idx[b0:b0 + block]]
        with np.errstate(all="ignore"):
            d = [Q[:, None, a] - X[None, :, a] for a in range(3)]
            M = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < r2f
        M &= fin[q_idx[b0:b0 + block], None]
        cnt[b0:b0 + block] = M.sum(1)
        cols.append(cand[np.nonzero(M)[1]])
    ptr = np.concatenate([[0], np.cumsum(cnt)])
    return ptr, (np.concatenate(cols) if cols else np.zeros(0, np.int64))


def _segment_sum(a, ptr):
    """Sums of a's rows over the CSR segments (empty segments: 0)."""
    cnt = np.diff(ptr)
    out = np.zeros((len(cnt),) + a.shape[1:], a.dtype)
    live = cnt > 0
    if live.any():
        out[live] = np.add.reduceat(a, ptr[:-1][live], axis=0)
    return out


# ---------------------------------------------------------------- the independent plane
def plane(xyz, ptr, idx):
    """dict of per-query arrays: cnt, cen [q,3], n [q,3], curv, lam [q,3] (ascending, of the covariance sum), kappa, kappa1, curv_cond,
    curv_cond1, usable (cnt >= 3 and l1 - l0 above the solver's rounding).  Rows with cnt < 3 hold NaN."""
    X = np.asarray(xyz, np.float32).reshape(-1, 3)[idx].astype(np.longdouble)
    cnt = np.diff(ptr)
    rep = np.repeat(np.arange(len(cnt)), cnt)
    with np.errstate(all="ignore"):
        cen = _segment_sum(X, ptr) / cnt[:, None].astype(np.longdouble)
        D = X - cen[rep]
        prod = np.stack([D[:, 0] * D[:, 0], D[:, 0] * D[:, 1], D[:, 0] * D[:, 2], D[:, 1] * D[:, 1], D[:, 1] * D[:, 2], D[:, 2] * D[:, 2]], 1)
        S = _segment_sum(prod, ptr).astype(np.float64)
    cov = S[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    ok = cnt >= 3
    lam = np.full((len(cnt), 3), np.nan)
    n = np.full((len(cnt), 3), np.nan)
    if ok.any():
        w, v = np.linalg.eigh(cov[ok])
        lam[ok], n[ok] = w, v[:, :, 0]
    cen64 = cen.astype(np.float64)
    with np.errstate(all="ignore"):
        tr = lam.sum(1)
        gap = lam[:, 1] - lam[:, 0]
        usable = ok & (gap > 4.0 * E64 * lam[:, 2])
        shift = cnt * (cen64 * cen64).sum(1)
        kappa = np.where(usable, lam[:, 2] / gap, np.inf)
        kappa1 = np.where(usable, (lam[:, 2] + shift) / gap, np.inf)
        curv = np.where(tr > 0.0, np.abs(lam[:, 0]) / tr, 0.0)
        curv_cond = np.where(tr > 0.0, lam[:, 2] / tr, np.inf)
        curv_cond1 = np.where(tr > 0.0, (lam[:, 2] + shift) / tr, np.inf)
    curv = np.where(ok, curv, np.nan)
    return dict(cnt=cnt, cen=cen64, n=n, curv=curv, lam=lam, kappa=kappa, kappa1=kappa1, curv_cond=curv_cond, curv_cond1=curv_cond1,
                usable=usable)


def sign_free_error(got, ref):
    """max |got - (+-)ref| per row, the better of the two signs."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.minimum(np.abs(got - ref).max(1), np.abs(got + ref).max(1))


# ---------------------------------------------------------------- the independent polynomial fit
def fit(xyz, ptr, idx, pl, r, order, queries=None):
    """MLS of the given order on the independent plane: (point [q,3], normal [q,3] unnormalised, cond [q] of P W P^T; 0 where the
    neighbourhood has fewer than (order + 1)(order + 2) / 2 points and the plane's projection stands).  float64."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    q_idx = np.arange(len(xyz)) if queries is None else np.asarray(queries, np.int64).ravel()
    nc = (order + 1) * (order + 2) // 2
    p = xyz[q_idx].astype(np.float64)
    n, cen = pl["n"], pl["cen"]
    with np.errstate(all="ignore"):
        dist = ((p - cen) * n).sum(1)
        pt = p - dist[:, None] * n
        v = unit_orthogonal(np.nan_to_num(n))
        u = _cross(n, v)
    point, normal, cond = pt.copy(), n.copy(), np.zeros(len(q_idx))
    if order == 0:
        return point, normal, cond
    gauss = float(r) * float(r)
    for k in np.nonzero((pl["cnt"] >= nc) & np.isfinite(n).all(1))[0]:
        E = xyz[idx[ptr[k]:ptr[k + 1]]].astype(np.float64) - pt[k]
        sw = np.sqrt(np.exp(-(E * E).sum(1) / gauss))
        P = _terms(E @ u[k], E @ v[k], order)
        c, _, _, s = np.linalg.lstsq(sw[:, None] * P, sw * (E @ n[k]), rcond=None)
        cond[k] = (s[0] / s[-1]) ** 2 if s[-1] > 0.0 else np.inf
        point[k] = pt[k] + c[0] * n[k]
        normal[k] = n[k] - (c[order + 1] * u[k] + c[1] * v[k])
    return point, normal, cond


# ---------------------------------------------------------------- the branch census
def one_pass_cov(xyz, ptr, idx):
    """normal_from_sums' covariance E[xx^T] - cc^T in double from the nine sums."""
    X = np.asarray(xyz, np.float32).reshape(-1, 3)[idx].astype(np.float64)
    cnt = np.diff(ptr).astype(np.float64)
    with np.errstate(all="ignore"):
        prod = np.stack([X[:, 0] * X[:, 0], X[:, 0] * X[:, 1], X[:, 0] * X[:, 2], X[:, 1] * X[:, 1], X[:, 1] * X[:, 2], X[:, 2] * X[:, 2]], 1)
        a = _segment_sum(prod, ptr) / cnt[:, None]
        c = _segment_sum(X, ptr) / cnt[:, None]
        pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        S = np.stack([a[:, t] - c[:, i] * c[:, j] for t, (i, j) in enumerate(pairs)], 1)
    return S[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def census_one_pass(xyz, ptr, idx):
    cen = {}
    n, curv = plane_from_cov(one_pass_cov(xyz, ptr, idx), cen)
    cen["cnt"] = np.diff(ptr)
    return n, curv, cen


# ---------------------------------------------------------------- exactness under Fraction
def _exact(fr):
    return Fraction(float(fr)) == fr


def _sums_exact(terms):
    """Every term and every partial sum, in any order, is a double: multiples of one power of two, their magnitudes' sum below 2^53 of it."""
    den = max(t.denominator for t in terms)
    return den & (den - 1) == 0 and sum(abs(t) for t in terms) * den < 2 ** 53


def exact_two_pass(pts):
    """True if the centroid, every de-meaned difference, every product and every partial sum of the two-pass covariance of these
    points is a double -- in whatever order they are added, fused or not."""
    P = [[Fraction(float(v)) for v in row] for row in np.asarray(pts, np.float64)]
    n = len(P)
    ok = all(_sums_exact([p[a] for p in P]) for a in range(3))
    cen = [sum(p[a] for p in P) / n for a in range(3)]
    ok &= all(_exact(c) for c in cen) and all(_exact(p[a] - cen[a]) for p in P for a in range(3))
    for a in range(3):
        for b in range(a, 3):
            ok &= _sums_exact([(p[a] - cen[a]) * (p[b] - cen[b]) for p in P])
    return bool(ok)


def exact_one_pass(pts):
    """The same for the nine sums, their division by the count and E[xx^T] - cc^T."""
    P = [[Fraction(float(v)) for v in row] for row in np.asarray(pts, np.float64)]
    n = len(P)
    ok = all(_sums_exact([p[a] for p in P]) for a in range(3))
    cen = [sum(p[a] for p in P) / n for a in range(3)]
    ok &= all(_exact(c) for c in cen)
    for a in range(3):
        for b in range(a, 3):
            m = sum(p[a] * p[b] for p in P) / n
            ok &= _sums_exact([p[a] * p[b] for p in P]) and _exact(m) and _exact(cen[a] * cen[b]) and _exact(m - cen[a] * cen[b])
    return bool(ok)


def exact_covariance(pts):
    """The two-pass covariance sum as Fractions (row-major 3 x 3)."""
    P = [[Fraction(float(v)) for v in row] for row in np.asarray(pts, np.float64)]
    n = len(P)
    cen = [sum(p[a] for p in P) / n for a in range(3)]
    return [[sum((p[a] - cen[a]) * (p[b] - cen[b]) for p in P) for b in range(3)] for a in range(3)]


# ---------------------------------------------------------------- the lattice fixture
def _grid(xs, ys, zs):
    return [(x, y, z) for x in xs for y in ys for z in zs]


def _clusters():
    q = [0.0, 0.5, 1.0, 1.5]
    bump = lambda x, y: 0.25 if x in (0.5, 1.0) and y in (0.25, 0.5) else 0.0
    return [
        # 1: axis planes, 16 points each (exact normals +-e_i, curvature 0, the c0 path; z = c: unitOrthogonal's second form)
        ("plane_x", (-512, 64, 512), [(0.0, y, z) for y in q for z in (0.0, 0.25, 0.75, 1.0)]),
        ("plane_y", (-448, -64, 528), [(x, 0.0, z) for x in q for z in (0.0, 0.25, 0.75, 1.0)]),
        ("plane_z", (-384, 128, 544), [(x, y, 0.0) for x in q for y in (0.0, 0.25, 0.75, 1.0)]),
        ("plane_z_far", (1024, -1024, 1024), [(x, y, 0.0) for x in q for y in (0.0, 0.25, 0.75, 1.0)]),
        # 2: a plane at 45 degrees, x = z
        ("plane_45", (-320, 16, 560), [(a, b, a) for a in q for b in (0.0, 0.25, 0.5, 1.0)]),
        # 3: a two-layer slab
        ("slab", (-256, -32, 576), _grid(q, (0.0, 1.0), (0.0,)) + _grid(q, (0.25, 0.75), (0.25,))),
        # 4: a bumped patch whose xz / yz moments vanish: n = +-z exactly, orders 1 / 2 have something to fit
        ("bumped", (-192, 48, 592), [(x, y, bump(x, y)) for x in q for y in (0.0, 0.25, 0.5, 0.75)]),
        # 5: 3, 4, 5, 6 points: the order-2 NC boundary
        ("three", (-128, 80, 608), [(0.0, 0.0, 0.0), (1.0, 0.0, 0.25), (0.0, 1.0, 0.5)]),
        ("four", (-64, -96, 624), [(0.0, 0.0, 0.0), (1.0, 0.0, 0.25), (0.0, 1.0, 0.5), (1.0, 1.25, 0.0)]),
        ("five", (0, 112, 640), [(0.0, 0.0, 0.0), (1.0, 0.0, 0.25), (0.0, 1.0, 0.5), (1.0, 1.25, 0.0), (0.5, 0.25, 0.25)]),
        ("six", (64, -16, 656), [(0.0, 0.0, 0.0), (1.0, 0.0, 0.25), (0.0, 1.0, 0.5), (1.0, 1.25, 0.0), (0.5, 0.25, 0.25), (1.5, 0.75, 0.0)]),
        # 6 - 8: no plane (NaN normal)
        ("line5", (128, 32, 672), [(0.25 * k, 0.25 * k, 0.0) for k in range(5)]),
        ("line4", (192, -48, 688), [(0.5 * k, 0.0, 0.25 * k) for k in range(4)]),
        ("repeated4", (256, 96, 704), [(0.5, 0.25, 0.75)] * 4),
        ("cube", (320, -80, 720), _grid((0.0, 1.0), (0.0, 1.0), (0.0, 1.0))),
        # 9: a repeated smallest eigenvalue (kappa infinite)
        ("prism", (384, 0, 736), _grid((0.0, 0.5), (0.0, 0.5), (0.0, 0.5, 1.0))),
        # 10: a 3 x 2 footprint with bumped heights: P W P^T of order 2 has rank 5
        ("footprint32", (448, 64, 752), [(0.0, 0.0, 0.0), (0.5, 0.0, 0.25), (1.0, 0.0, 0.0), (0.0, 0.5, 0.0), (0.5, 0.5, 0.0), (1.0, 0.5, 0.25)]),
        # the one-pass kernels' r0 <= 0 fallback: see fallback_cluster()
        ("fallback1", FALLBACK_ORIGIN, FALLBACK_POINTS),
        ("pair_a", (512, -64, 768), [(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)]),
        ("pair_b", (-512, -128, 784), [(0.0, 0.0, 0.0), (0.0, 0.25, 1.0)]),
        # the radius test is strict: the first and the last point are exactly r = 2.5 apart (1.5^2 + 2^2) and do not see each other,
        # so each has 2 neighbours and only the middle one, with 3, is emitted
        ("rim", (576, 128, 800), [(0.0, 0.0, 0.0), (0.0, 0.25, 0.0), (1.5, 2.0, 0.0)]),
    ]


# A planar cluster of 6 points far from the origin.  Six is no power of two, so the nine (exact) sums' division rounds and the one-pass
# covariance of these coplanar points has a smallest eigenvalue of rounding size, here below zero: |c0| >= eps and the trigonometric
# r0 = -5.5e-10, six orders below what the last bits of atan2 / cos / sin can move (the library is built without contraction, so
# the covariance has the CPU's bits).  computeRoots then falls back to computeRoots2 and the curvature is exactly 0; without the
# fallback it is ~1e-10.
FALLBACK_ORIGIN = (-1024, 1024, 768)
FALLBACK_POINTS = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.25), (0.0, 1.0, 0.5), (1.0, 1.0, 0.75), (0.5, 0.25, 0.25), (1.0, 0.5, 0.5)]

EXACT_PLANES = {"plane_x": 0, "plane_y": 1, "plane_z": 2, "plane_z_far": 2}        # cluster -> the axis of its normal
NO_PLANE = ("line5", "line4", "repeated4", "cube")              # NaN normal in the restated PCL, two-pass and one-pass (both exact)
UNDECIDED = ("prism",)          # NaN or finite on the last bit of cos / sin: in no value or pattern comparison
RANK_DEFICIENT = ("footprint32",)


def lattice_fixture():
    """(xyz float32 [n,3], {cluster name: indices}).  A few non-finite points lie between the clusters."""
    rows, where = [], {}
    bad = [[np.nan, 0.0, 600.0], [np.inf, 1.0, 2.0], [0.0, -np.inf, 5.0], [-320.0, 16.0, np.nan]]
    for k, (name, org, pts) in enumerate(_clusters()):
        if k % 5 == 2:
            rows.append(bad[(k // 5) % len(bad)])
        where[name] = np.arange(len(rows), len(rows) + len(pts))
        rows.extend([[org[0] + p[0], org[1] + p[1], org[2] + p[2]] for p in pts])
    xyz = np.array(rows, np.float64)
    assert np.array_equal(xyz.astype(np.float32).astype(np.float64), xyz, equal_nan=True)
    return xyz.astype(np.float32), where


def lattice_ref_normals(xyz, seed=7):
    """Reference normals for the MLS flip on the lattice fixture: exact (+-1, +-1, +-1) / 2-ish directions never orthogonal to an
    axis normal, a few NaN (those never flip)."""
    rng = np.random.default_rng(seed)
    ref = np.zeros((len(xyz), 4), np.float32)
    ref[:, :3] = rng.choice([-1.0, 1.0], (len(xyz), 3)) * [0.5, 0.25, 1.0]
    ref[rng.choice(len(xyz), 6, replace=False)] = np.nan
    return ref


# ---------------------------------------------------------------- fixtures with their references, and the comparisons
FAR_SHIFT = (5 * 4096.0, 5 * 4096.0, 12 * 4096.0)      # a millimetre rig: x, y ~ 2e4, z ~ 5e4; float32 keeps 2^-8 there
_fixtures = {}


def fixture(name):
    """dict(xyz, r, ref (normals for the MLS flip), ptr, idx, pl (plane()), fits {order: fit()}, where (lattice: cluster -> indices),
    mask {order: rows compared by value}) of "lattice", "dense" (surface_cloud(6000, 2), r 2.5), "sparse" (surface_cloud(3000, 3),
    r 1.2), "far" (dense, shifted by FAR_SHIFT) or "sheet" (the 3000 points around the middle of the CPU oracle's cloud of
    test_gpu_cloud_filter's thin-sheet pair, r 9).  Computed once."""
    if name in _fixtures:
        return _fixtures[name]
    where = {}
    if name == "lattice":
        (xyz, where), r = lattice_fixture(), R_LATTICE
        ref = lattice_ref_normals(xyz)
    elif name == "sheet":
        from oracle import oracle as orc
        from reconstruction_amd import synth
        from test_gpu_cloud_filter import PAIRS_W
        from test_gpu_mls import ref_normals
        cloud = orc.match_pair(synth.config_small(**PAIRS_W[5]))["xyz"].astype(np.float32)
        cloud = cloud[np.isfinite(cloud).all(1)]
        d = np.abs(cloud[:, :2] - np.median(cloud[:, :2], axis=0)).max(1)
        xyz, r = cloud[np.sort(np.argsort(d, kind="stable")[:3000])], 9.0
        ref = ref_normals(xyz, 5)
    else:
        from test_gpu_mls import ref_normals, surface_cloud
        n, seed, r = (3000, 3, 1.2) if name == "sparse" else (6000, 2, 2.5)
        xyz = surface_cloud(n, seed)
        ref = ref_normals(xyz, seed)
        if name == "far":
            xyz = (xyz.astype(np.float64) + FAR_SHIFT).astype(np.float32)
    ptr, idx = neighbourhoods(xyz, r)
    pl = plane(xyz, ptr, idx)
    fx = dict(name=name, xyz=xyz, r=r, ref=ref, ptr=ptr, idx=idx, pl=pl, where=where, fits={o: fit(xyz, ptr, idx, pl, r, o) for o in (0, 1, 2)})
    emitted = pl["cnt"] >= 3
    base = emitted & pl["usable"]
    for c in UNDECIDED:
        if c in where:
            base[where[c]] = False
    fx["emitted"] = emitted
    fx["mask"] = {o: base.copy() for o in (0, 1, 2)}
    for c in RANK_DEFICIENT:
        if c in where:
            fx["mask"][2][where[c]] = False
    _fixtures[name] = fx
    return fx


def scatter(n, index, *arrays):
    """Compacted outputs (rows for the input indices `index`) back at their input rows, NaN elsewhere."""
    out = []
    for a in arrays:
        full = np.full((n,) + a.shape[1:], np.nan, np.float64)
        full[index] = a
        out.append(full)
    return out


def compare_normals(fx, got4, one_pass, mask=None):
    """{bound name: (err, rnd, cond)} of order-0 normals and curvatures got4 ([n,4], input rows) on the compared rows."""
    pl = fx["pl"]
    m = fx["mask"][0] if mask is None else mask
    g = np.asarray(got4, np.float64)[m]
    with np.errstate(all="ignore"):
        e_n = np.where(np.isfinite(g[:, :3]).all(1), sign_free_error(g[:, :3], pl["n"][m]), np.inf)
        e_c = np.where(np.isfinite(g[:, 3]), np.abs(g[:, 3] - pl["curv"][m]), np.inf)
    s = "1" if one_pass else "2"
    return {"normal" + s: (e_n, U32, E64 * pl["kappa" + ("1" if one_pass else "")][m]),
            "curv" + s: (e_c, half_ulp32(pl["curv"][m]), E64 * pl["curv_cond" + ("1" if one_pass else "")][m])}


def compare_mls(fx, order, gx, gn, mask=None):
    """The same for MLS of one order: positions gx [n,3], normals + curvature gn [n,4] at the input rows."""
    pl = fx["pl"]
    m = fx["mask"][order] if mask is None else mask
    point, normal, cond = (a[m] for a in fx["fits"][order])
    gx, gn = np.asarray(gx, np.float64)[m], np.asarray(gn, np.float64)[m]
    with np.errstate(all="ignore"):
        c = E64 * (pl["kappa"][m] + cond)
        e_p = np.where(np.isfinite(gx), np.abs(gx - point), np.inf)
        out = {"pos": (e_p, half_ulp32(point), (c * fx["r"])[:, None] + E64 * np.abs(point)),
               "curv2": (np.where(np.isfinite(gn[:, 3]), np.abs(gn[:, 3] - pl["curv"][m]), np.inf), half_ulp32(pl["curv"][m]), E64 * pl["curv_cond"][m])}
        if order == 0:
            out["normal2"] = (np.where(np.isfinite(gn[:, :3]).all(1), sign_free_error(gn[:, :3], normal), np.inf), U32, E64 * pl["kappa"][m])
        else:
            sgn = np.where((gn[:, :3] * normal).sum(1) < 0.0, -1.0, 1.0)[:, None]
            e_n = np.where(np.isfinite(gn[:, :3]), np.abs(gn[:, :3] - sgn * normal), np.inf)
            out["fitnormal"] = (e_n, U32 * np.maximum(1.0, np.abs(normal)), np.broadcast_to(c[:, None], e_n.shape))
    return out


def worst_ratio(cmp, mult=KERNEL_K):
    """{bound name: the largest err / bound} (bound with mult x K; 0 / 0 counts as 0)."""
    out = {}
    for which, (err, rnd, cond) in cmp.items():
        with np.errstate(all="ignore"):
            b = bound(rnd, cond, which, mult)
            ratio = np.where(err <= b, np.where(b > 0.0, err / b, 0.0), np.where(np.isfinite(b), err / b, 0.0))
        out[which] = float(np.max(np.nan_to_num(ratio, nan=0.0, posinf=np.inf), initial=0.0))
    return out
