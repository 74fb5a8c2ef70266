"""The radius outlier pass of the cloud filter (csrc/k_filter_outrem.hip; pcl::RadiusOutlierRemoval, CCloudOptimization.cpp:90-96), restated
by brute force in numpy float32 from the definition in include/rsm.h -- and the cloud that motivates the pass.  Test infrastructure only.

  S = the cloud handed in (the survivors of the outlier removal before the pass), S_f its finite points;
  count(p) = #{ q in S_f : fdist2(p, q) < fl32(r r) }: p itself counts, coincident points count once each, a non-finite p has count 0;
  p stays iff count(p) > min_neighbors.
The membership test is tests/cloud_probes.py's (fdist2, accept(..., "radius")): the one the grid's cell rule is proven against.
"""
import numpy as np

from cloud_probes import accept, fdist2

F32 = np.float32
INT32_MAX = 2 ** 31 - 1


def radius_counts(xyz, radius, cap=None, chunk=512, queries=None):
    """count(p) for every point of xyz [n, 3] (cast to float32), int64 [n]; with cap, min(count, cap) -- what rsm_stage_radius_count returns.
    queries: count these points against the cloud xyz instead (a sample of a large cloud)."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    fin = np.isfinite(xyz).all(1)
    Sf = xyz[fin]
    xyz = xyz if queries is None else np.asarray(queries, F32).reshape(-1, 3)
    out = np.zeros(len(xyz), np.int64)
    with np.errstate(all="ignore"):
        for s in range(0, len(xyz), chunk):
            P = xyz[s:s + chunk, None, :]
            out[s:s + chunk] = accept(fdist2(P, Sf[None]), radius, "radius").sum(1)   # (a non-finite p: every comparison is false)
    return out if cap is None else np.minimum(out, int(cap))


def radius_counts_tree(xyz, radius):
    """The same counts for a cloud too large for n^2 comparisons in a test: the float32 membership test on the candidates a k-d tree finds
    within 1.001 radius in double (a superset: float32 rounding moves a distance by parts in 10^7); test_outrem_cpu.py holds it to
    radius_counts."""
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    fin = np.isfinite(xyz).all(1)
    Sf = xyz[fin]
    out = np.zeros(len(xyz), np.int64)
    pairs = cKDTree(Sf.astype(np.float64)).query_pairs(1.001 * float(radius), output_type="ndarray")
    inside = accept(fdist2(Sf[pairs[:, 0]], Sf[pairs[:, 1]]), radius, "radius")
    c = 1 + np.bincount(pairs[inside].ravel(), minlength=len(Sf))      # (the point itself: fdist2 = 0 < r2)
    out[fin] = c
    return out


def radius_keep(xyz, min_neighbors, radius):
    """The pass's verdict on the cloud xyz as S: bool [n]."""
    return radius_counts(xyz, radius) > int(min_neighbors)


def report(xyz, min_neighbors, radius):
    """What rsm_filter_last_outrem says of the pass on S = xyz, route apart: (points_in, removed, nonfinite among the removed)."""
    keep = radius_keep(xyz, min_neighbors, radius)
    fin = np.isfinite(np.asarray(xyz, F32).reshape(-1, 3)).all(1)
    return len(keep), int((~keep).sum()), int((~keep & ~fin).sum())


# ---- hand-worked cases: (name, xyz, radius, the counts worked out by hand)
def hand_cases():
    two = [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]
    nan, inf = float("nan"), float("inf")
    odd = [[0.0, 0.0, 0.0], [nan, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, inf, 0.0], [0.0, 0.5, 0.0]]
    return [("d2 = r2 is not inside", two, 2.0, [1, 1]),
            ("one ulp below", [[0.0, 0.0, 0.0], [float(np.nextafter(F32(2.0), F32(0.0))), 0.0, 0.0]], 2.0, [2, 2]),
            ("a single point", [[1.0, 2.0, 3.0]], 2.0, [1]),
            ("300 coincident points", [[7.0, -3.0, 50.0]] * 300, 0.25, [300] * 300),
            ("non-finite points count 0 and are never counted", odd, 2.0, [3, 0, 3, 0, 3])]


# ---- pairs at the cell boundaries of the grid: the radius-cell grid over a box whose low corner is (o, o, o) has its boundaries at
# o + j grid_edge(r); a point within a few ulps of one and its partner within a few ulps of distance r on the other side, one pair per
# row of cells.  Some of the pairs are inside the radius, some exactly on it, some outside: a lost neighbour or a wrong comparison shows
# as a count that is one off.
def boundary_cloud(r, o, js=(1, 2, 3, 5, 12, 41, 100), k=2):
    from cloud_probes import _ulps, grid_edge
    h = float(F32(r))
    o32 = F32(o)
    pts = [[o32, o32, o32]]
    z0 = F32(float(o32) + 1.5 * h)
    row = 0
    for j in js:
        for a in _ulps(np.array([float(o32) + j * grid_edge(r)], F32), k)[0]:
            for sgn in (1.0, -1.0):
                for b in _ulps(np.array([float(a) + sgn * h], F32), k + 1)[0]:
                    y = F32(float(o32) + (4 * row + 1.5) * h)
                    row += 1
                    pts += [[a, y, z0], [b, y, z0]]
    return np.asarray(pts, F32)


# ---- the motivating cloud: a clump of wrong matches denser than the surface passes the statistical removal whatever its size
SHEET_W, SHEET_H, SPACING = 48, 40, 0.5
CLUMP_N, CLUMP_SIGMA, CLUMP_AT = 30, 0.15, (10.0, 8.0, 38.0)
STRAGGLERS = 6
NONFINITE_AT = 100


def clump_cloud(seed=5):
    """A 48 x 40 sheet at spacing 0.5, z = 50 + 0.3 sin(x) + 0.02 noise; a clump of 30 points (sigma 0.15) 12 units in front of it; six
    stragglers far from both; a NaN point and an inf point at index 100.  Returns (xyz float32 [1958, 3], part int [1958]: 0 the sheet,
    1 the clump, 2 the stragglers, 3 the non-finite points)."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(SHEET_W) * SPACING, np.arange(SHEET_H) * SPACING)
    x, y = gx.ravel(), gy.ravel()
    sheet = np.stack([x, y, 50.0 + 0.3 * np.sin(x) + 0.02 * rng.standard_normal(len(x))], 1)
    clump = np.asarray(CLUMP_AT) + CLUMP_SIGMA * rng.standard_normal((CLUMP_N, 3))
    # the stragglers: single points 15 .. 40 units off the sheet's plane, at least 8 units from one another and from the clump
    far = np.stack([np.linspace(-6.0, 30.0, STRAGGLERS), rng.uniform(-6.0, 26.0, STRAGGLERS), 50.0 + rng.choice([-1.0, 1.0], STRAGGLERS) * rng.uniform(15.0, 40.0, STRAGGLERS)], 1)
    xyz = np.concatenate([sheet, clump, far])
    part = np.concatenate([np.zeros(len(sheet), int), np.ones(CLUMP_N, int), np.full(STRAGGLERS, 2)])
    bad = np.array([[np.nan, 1.0, 2.0], [3.0, np.inf, 50.0]])
    xyz = np.concatenate([xyz[:NONFINITE_AT], bad, xyz[NONFINITE_AT:]])
    part = np.concatenate([part[:NONFINITE_AT], [3, 3], part[NONFINITE_AT:]])
    return xyz.astype(F32), part
