"""The radius outlier pass's restatement (tests/outrem_restatement.py) held to hand-worked cases and to scipy's ball query, and the cloud
that motivates the pass held to what it claims: a clump of wrong matches denser than the surface passes the statistical outlier removal
whole and falls to the radius count whole.  No GPU: tests/test_gpu_cloud_outrem.py runs the same clouds through the kernels."""
import numpy as np
import pytest

import cloud_probes as cp
import outrem_restatement as R
from oracle import oracle as orc

F32 = np.float32


@pytest.mark.parametrize("case", range(len(R.hand_cases())))
def test_hand_worked_counts(case):
    name, xyz, radius, want = R.hand_cases()[case]
    assert R.radius_counts(xyz, radius).tolist() == want, name
    # min_neighbors = 0: the finite points stay, the others go
    assert R.radius_keep(xyz, 0, radius).tolist() == np.isfinite(np.asarray(xyz, F32)).all(1).tolist()


def test_counts_equal_scipys_ball_query_away_from_ties():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(21)
    n, radius = 800, 1.3
    xyz = np.stack([rng.uniform(0, 20, n), rng.uniform(0, 15, n), 30.0 + rng.normal(0, 0.2, n)], 1).astype(F32)
    r2 = float(F32(radius * radius))
    d2 = np.concatenate([cp.fdist2(xyz[s:s + 500, None, :], xyz[None]).ravel() for s in range(0, n, 500)]).astype(np.float64)
    assert np.abs(d2 - r2).min() > 1e-5 * r2            # no squared distance near r2: float32 and double agree on every comparison
    want = [len(v) for v in cKDTree(xyz.astype(np.float64)).query_ball_point(xyz.astype(np.float64), radius)]
    got = R.radius_counts(xyz, radius)
    assert got.tolist() == want and 1 <= got.min() < 10 < got.max()


def test_the_clump_passes_the_statistical_removal_and_falls_to_the_radius_count():
    xyz, part = R.clump_cloud()
    assert len(xyz) == 1958 and not np.isfinite(xyz[100:102]).all(1).any() and np.isfinite(np.delete(xyz, [100, 101], 0)).all()
    keep, _, _ = orc.sor_filter(xyz, 8, 1.0)
    assert keep[part == 1].all() and keep[part == 3].all()         # the whole clump and both non-finite points pass
    assert not keep[part == 2].any() and keep[part == 0].all()     # the six stragglers go, and only they
    assert keep.sum() == 1952
    S, ps = xyz[keep], part[keep]
    c = R.radius_counts(S, 2.0)
    k = c > 40
    assert not k[ps == 1].any() and not k[ps == 3].any()           # (40, 2.0): the clump and the non-finite points go ...
    gone = 1.0 - k[ps == 0].mean()
    assert 0.20 < gone < 0.30                                      # ... and the sheet's rim
    gx, gy = S[ps == 0][:, 0] / R.SPACING, S[ps == 0][:, 1] / R.SPACING
    rim = np.minimum(np.minimum(gx, R.SHEET_W - 1 - gx), np.minimum(gy, R.SHEET_H - 1 - gy))
    assert rim[~k[ps == 0]].max() < rim[k[ps == 0]].min() + 1.5    # what goes is the outermost rings
    assert k.sum() == 1428 and c.max() == 45
    k = R.radius_keep(S, 12, 1.0)
    assert k.sum() == 30 and k[ps == 1].all()                      # (12, 1.0) keeps exactly the clump
    assert R.report(S, 40, 2.0) == (1952, 1952 - 1428, 2)


@pytest.mark.parametrize("min_neighbors,radius", [(40, 2.0), (12, 1.0)])
def test_a_capped_count_decides_as_the_full_count(min_neighbors, radius):
    xyz, _ = R.clump_cloud()
    full = R.radius_counts(xyz, radius)
    for cap in (1, min_neighbors + 1, R.INT32_MAX):
        capped = R.radius_counts(xyz, radius, cap)
        assert np.array_equal(capped, np.minimum(full, cap))
    assert np.array_equal(R.radius_counts(xyz, radius, min_neighbors + 1) > min_neighbors, full > min_neighbors)
    assert np.array_equal(R.radius_counts(xyz, radius, 1), np.isfinite(xyz).all(1).astype(np.int64))


def test_the_tree_form_of_the_restatement_equals_the_brute_force():
    xyz, _ = R.clump_cloud()
    for radius in (1.0, 2.0, 2.5):
        assert np.array_equal(R.radius_counts_tree(xyz, radius), R.radius_counts(xyz, radius))
    for name, pts, radius, want in R.hand_cases():
        assert R.radius_counts_tree(pts, radius).tolist() == want, name
    for r, o in ((2.0, 0), (2.5, -37.7)):                      # pairs within ulps of the radius, on both sides of it
        xyz = R.boundary_cloud(r, o)
        assert np.array_equal(R.radius_counts_tree(xyz, r), R.radius_counts(xyz, r))


PROBE_RADII, PROBE_ORIGINS = (0.5, 2.0, 2.5), (0, 1000.25, -37.7)


@pytest.mark.parametrize("o", PROBE_ORIGINS)
@pytest.mark.parametrize("r", PROBE_RADII)
def test_boundary_clouds_put_pairs_on_both_sides_of_the_radius_across_cells(r, o):
    """tests/cloud_probes.py's radius_probe_cloud needs an accepted pair the float cell rule puts two cells apart; at the origins 0 and
    1000.25 that rule rounds nothing and no such pair exists (the generator says so), so the GPU test runs boundary_cloud at all nine
    (r, o) and the probe cloud where there is one.  Here: the boundary cloud has pairs inside, on and outside the radius, in different
    cells of the grid the count walks."""
    xyz = R.boundary_cloud(r, o)
    p, q = xyz[1::2], xyz[2::2]
    d2 = cp.fdist2(p, q)
    r2 = F32(float(r) * float(r))
    assert (d2 < r2).sum() > 20 and (d2 == r2).sum() > 5 and (d2 > r2).sum() > 20
    lo, n = xyz.min(0), cp.dims("fixed", r, xyz.min(0), xyz.max(0))
    gap = np.abs(cp.cells("fixed", p[:, 0], lo[0], r, n[0]) - cp.cells("fixed", q[:, 0], lo[0], r, n[0]))
    assert (gap[d2 < r2] == 1).sum() > 20 and gap[d2 < r2].max() <= 1
    c = R.radius_counts(xyz, r)
    assert set(c[1:].tolist()) == {1, 2} and np.array_equal(c[1::2] == 2, d2 < r2)


def test_which_probe_clouds_exist():
    built = {}
    for r in PROBE_RADII:
        for o in PROBE_ORIGINS:
            try:
                xyz, info = cp.radius_probe_cloud(r, o, clusters=12, jmax=4000)
                built[(r, o)] = info["lost"] > 0
            except AssertionError as e:
                assert "no straddling pair" in str(e)
                built[(r, o)] = False
    assert all(built[(r, -37.7)] for r in PROBE_RADII), built
