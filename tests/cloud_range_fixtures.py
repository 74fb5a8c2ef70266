"""Clouds for the per-pair filter's tests (plain numpy, no GPU): the bumpy sheet the filter tests share, and the clouds whose
neighbour distances span many octaves -- where the order of a double sum of float32 values starts to matter.

PCL and oracle/cloud_oracle.c add the square roots of a point's k nearest squared distances into a double one after the other, in
ascending order, and the per-point means into a double in point order.  A sum of float32 values in a double is free of rounding -- and
then of its order -- only while every value is a multiple of 2^q and the total stays below 2^(q + 53); `stats_fast_path` restates that
rule as the library's host applies it to the sums over the cloud."""
import itertools

import numpy as np

F32 = np.float32


def surface_cloud(n, seed, extent=60.0, outliers=200, duplicates=50):
    """A bumpy depth-map-like patch (anisotropic sampling as a perspective camera gives it), far and near outliers,
    exact duplicates, an isolated cluster smaller than k."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2)) * [extent, 0.7 * extent] - [extent / 2, 0.35 * extent]
    z = 600.0 + 6.0 * np.sin(u[:, 0] / 9.0) * np.cos(u[:, 1] / 7.0) + rng.normal(0, 0.03, n)
    xyz = np.c_[u * (z[:, None] / 600.0), z]
    idx = rng.choice(n, outliers, replace=False)
    xyz[idx] += rng.normal(0, 1.0, (outliers, 3)) * rng.choice([0.5, 3.0, 40.0], (outliers, 1))
    idx = rng.choice(n, duplicates, replace=False)
    xyz[idx] = xyz[rng.choice(n, duplicates)]
    xyz[:30] = [200.0, 150.0, 900.0] + rng.normal(0, 0.2, (30, 3))     # an island of 30 < k points
    xyz = xyz.astype(np.float32)
    xyz[40:44] = [[np.inf, 1.0, 2.0], [np.nan, np.nan, np.nan], [0.0, -np.inf, 5.0], [1.0, 2.0, np.nan]]   # d == 0 gives 1/0 (.cpp:745)
    return xyz


# ---- the tie cloud: nine points, k = 8, whose first point's sum of distances rounds differently in different orders
TIE_K = 8
TIE_T = F32(0.4 * 2.0 ** -50)
TIE_FAR = F32(1.5 + 2.0 ** -22)
TIE_DIST0 = float.fromhex("0x1.a00002p-1")    # the oracle's mean distance of the origin: the ascending sum's


def tie_cloud():
    """The origin, two near-duplicates of it at +-t (squared distance ~2^-102: below the trimmed square root's domain), five points
    a unit away and one at 1.5 + 2^-22.  The origin's sum 2 t + 5 + (1.5 + 2^-22) sits on a rounding boundary of the double and of
    the float32 mean: adding the two t before the ones or after them gives different float32 results."""
    t = TIE_T
    return np.array([[0, 0, 0], [t, 0, 0], [-t, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -TIE_FAR]], F32)


def tie_values():
    """The origin's seven neighbour distances below the largest, ascending, and the largest."""
    return [TIE_T, TIE_T, F32(1), F32(1), F32(1), F32(1), F32(1)], TIE_FAR


def sequential_mean(values, last, k):
    """float32(((v0 + v1) + ...) + last) / k) in double, as PCL's loop forms a point's mean distance."""
    s = 0.0
    for v in values:
        s += float(v)
    s += float(last)
    return float(F32(s / k))


def tie_orders():
    """{order of the seven values: the float32 mean it gives}, every distinct order."""
    vals, last = tie_values()
    return {p: sequential_mean(p, last, TIE_K) for p in set(itertools.permutations(vals))}


# ---- the wide clouds: surface_cloud with one thing added that stretches the range of the distances
WIDE_BASES = [(3000, 3, 20), (6000, 2, 100)]     # (n, seed, k)
WIDE_VARIANTS = ["control", "far1e6", "far1e9", "far1e20", "tight", "tight_small", "underflow"]
WIDE_AT = 100      # first row a variant overwrites (behind the island and the non-finite rows)
_wide = {}


def wide_cloud(n, seed, k, variant):
    xyz = surface_cloud(n, seed)
    rng = np.random.default_rng(1000 + seed)
    if variant == "far1e6":
        xyz[WIDE_AT] = [3e5, -2e5, 1e6]
    elif variant == "far1e9":
        xyz[WIDE_AT] = [3e8, -2e8, 1e9]
    elif variant == "far1e20":
        xyz[WIDE_AT] = [0.0, 0.0, 1e20]                    # float32 squared distances to it: +inf
    elif variant in ("tight", "tight_small"):
        m = k + 5 if variant == "tight" else k - 3         # a near-duplicate cluster larger / smaller than k
        xyz[WIDE_AT:WIDE_AT + m] = (np.array([1e-3, 2e-3, 1e-3]) + rng.normal(0, 1e-9, (m, 3))).astype(F32)
    elif variant == "underflow":
        # twelve distinct points whose float32 squared distances to each other are subnormal (1e-22 apart) or 0 (1e-30 apart)
        pts = [[i * 1e-22, 0.0, 0.0] for i in range(6)] + [[0.0, j * 1e-30, 0.0] for j in range(1, 4)] + [[0.0, 0.0, -j * 1e-30] for j in range(1, 4)]
        xyz[WIDE_AT:WIDE_AT + 12] = np.array(pts, F32)
    else:
        assert variant == "control"
    return xyz


def wide_clouds():
    """[(name, xyz, k)]: every variant on both bases (built once, shared; treat as read-only)."""
    if not _wide:
        for n, seed, k in WIDE_BASES:
            for v in WIDE_VARIANTS:
                xyz = wide_cloud(n, seed, k, v)
                xyz.setflags(write=False)
                _wide["%s-n%d-k%d" % (v, n, k)] = (xyz, k)
    return [(name, xyz, k) for name, (xyz, k) in _wide.items()]


LONG_K = 4200      # more neighbours than the kernels' lists hold (2048 in the grid search's selection, 4096 in the whole-cloud search)


def long_sum_cloud():
    """surface_cloud(4500, 5) with 30 near-duplicates near the origin, for k = LONG_K: each of the 30 adds 29 distances of ~1e-9 and
    4171 of ~600 -- an order-dependent sum of more values than either list holds."""
    xyz = surface_cloud(4500, 5)
    rng = np.random.default_rng(77)
    xyz[WIDE_AT:WIDE_AT + 30] = (np.array([1e-3, 2e-3, 1e-3]) + rng.normal(0, 1e-9, (30, 3))).astype(F32)
    return xyz


_oracle = {}


def wide_oracle(name):
    """oracle.sor_filter of a wide cloud (computed once per process): (keep, dist, (mean, stddev, threshold))."""
    from oracle import oracle as orc
    if name not in _oracle:
        wide_clouds()
        xyz, k = _wide[name]
        _oracle[name] = orc.sor_filter(xyz, k, 1.0)
    return _oracle[name]


def dist2_f32(p, pts):
    """(dx dx + dy dy) + dz dz on float32 differences, as the oracle and the kernels form a squared distance."""
    d = np.asarray(p, F32)[None] - np.asarray(pts, F32)
    with np.errstate(over="ignore", under="ignore"):
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def knn_roots(xyz, i, k):
    """What PCL adds for point i: float32 square roots of its k smallest float32 squared distances to the other finite points,
    ascending (its own 0 left out)."""
    fin = np.isfinite(xyz).all(1)
    d2 = np.sort(dist2_f32(xyz[i], xyz[fin]))[1:k + 1]
    return np.sqrt(d2.astype(F32))


def sum_is_order_free(values):
    """The rule itself: every value a multiple of 2^q, the total below 2^(q + 53) -- no partial sum in any order rounds.  (The
    kernels test a stricter form per query -- q from the smallest positive value's exponent alone -- and add in PCL's order when
    it fails.)"""
    v = np.ascontiguousarray(values, F32)
    q = int(low_bit_exp(v).min())
    return q >= (1 << 40) or float(np.sum(v.astype(np.float64))) < 2.0 ** (q + 53)


# ---- the host's acceptance rule for the parallel sums over the cloud, restated
def low_bit_exp(v):
    """Exponent of the lowest set bit of each finite float32 (the largest q with v a multiple of 2^q); a huge value for 0."""
    u = np.ascontiguousarray(v, F32).view(np.uint32) & np.uint32(0x7fffffff)
    e = (u >> 23).astype(np.int64)
    m = (u & np.uint32(0x7fffff)).astype(np.int64)
    m = np.where(m != 0, m, 1 << 23)                          # (an empty mantissa field: the implicit bit is the lowest)
    tz = np.log2((m & -m).astype(np.float64)).astype(np.int64)   # trailing zeros
    q = np.where(e == 0, -149 + tz, (e - 150) + tz)
    return np.where(u == 0, np.int64(1 << 40), q)


def stats_fast_path(dist):
    """What decides whether the library takes the parallel sums of the per-point distances: (accepted, why not).  Accepted iff no
    distance is negative or NaN and no float32 square non-finite (`bad`), and each of the two totals -- over d and over float32(d d) --
    stays below 2^(q + 53), q the lowest set bit over its terms."""
    d = np.ascontiguousarray(dist, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        dd = (d * d).astype(F32)
    if (~(d >= 0)).any() or (~np.isfinite(dd)).any():
        return False, "bad"
    why = []
    for name, v in (("sum", d), ("sq_sum", dd)):
        q = int(low_bit_exp(v).min())
        total = float(np.sum(v.astype(np.float64)))
        if q < (1 << 40) and not total * (1.0 + 1e-9) < 2.0 ** (q + 53):
            why.append(name)
    return not why, "+".join(why)
