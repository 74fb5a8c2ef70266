"""The radius-cell grid of the cloud searches (csrc/cloud_grid.h) restated in numpy (tests/cloud_probes.py): an adversarial sweep
over cell boundaries finds pairs that the membership test accepts but the float cell rule before the fix puts two cells apart, and
none under the fixed rule.  No GPU."""
import numpy as np
import pytest

import cloud_probes as cp

F32 = np.float32


@pytest.fixture(scope="module")
def sweep():
    js = cp.sweep_js(np.random.default_rng(7), 200)
    return {(r, o, kind, rule): len(cp.straddles(rule, r, o, js, kind)) for r in cp.RADII for o in cp.ORIGINS
            for kind in ("radius", "knn") for rule in ("old", "new")}


@pytest.mark.parametrize("r", cp.RADII)
def test_the_old_rule_puts_accepted_pairs_two_cells_apart(sweep, r):
    found = {(o, kind): sweep[(r, o, kind, "old")] for o in cp.ORIGINS for kind in ("radius", "knn")}
    assert sum(found.values()) > 0, found
    assert sum(v for (o, kind), v in found.items() if kind == "knn") > 0, found


@pytest.mark.parametrize("r", cp.RADII)
def test_the_fixed_rule_keeps_every_accepted_pair_in_adjacent_cells(sweep, r):
    found = {(o, kind): sweep[(r, o, kind, "new")] for o in cp.ORIGINS for kind in ("radius", "knn")}
    assert sum(found.values()) == 0, found


@pytest.mark.parametrize("r,a,b,cells", [(2.5, -7.2500014, -4.750002, 13), (0.7, -7.8500013, -7.1500015, 43)])
def test_the_known_pairs(r, a, b, cells):
    """Grid origin -37.25: at radius 2.5 (the reference's m_mls_radius) fl32(-4.750002 + 37.25) = 32.5 exactly, cell 13 of 2.5 --
    two cells above -7.2500014's 11 -- at a float distance below r."""
    a, b, o = F32(a), F32(b), F32(-37.25)
    d = F32(b - a)
    assert d * d < F32(r * r)
    old = cp.cells("old", np.array([a, b]), o, r, cp.CAP)
    new = cp.cells("new", np.array([a, b]), o, r, cp.CAP)
    assert old[1] == cells and old[1] - old[0] == 2
    assert new[1] - new[0] == 1


@pytest.mark.parametrize("r", [0.1, 0.7, 2.5])
def test_clamping_at_the_cell_cap(r):
    """Boxes wider than 2^20 cells: the cell count stops at the cap, points beyond the last cell share it (clamping is
    non-expansive), and pairs across the last boundaries and beyond the box stay adjacent under the fixed rule."""
    o = F32(-1.0)
    far = F32(float(o) + 3.0 * cp.CAP * r)
    n = cp.dims("new", r, [o] * 3, [far] * 3)
    assert (n == cp.CAP).all()
    js = np.array([cp.CAP - 3, cp.CAP - 2, cp.CAP - 1, cp.CAP, cp.CAP + 1, 2 * cp.CAP, 3 * cp.CAP - 1])
    for kind in ("radius", "knn"):
        assert len(cp.straddles("new", r, o, js, kind, n=cp.CAP)) == 0
    v = (F32(o) + np.array([2.0 * cp.CAP, 2.5 * cp.CAP]) * r).astype(F32)
    assert (cp.cells("new", v, o, r, cp.CAP) == cp.CAP - 1).all() and (cp.cells("new", F32(-1e30), o, r, cp.CAP) == 0)


def test_one_cell_when_the_radius_exceeds_the_cloud():
    rng = np.random.default_rng(3)
    xyz = (rng.normal(0, 1.0, (50, 3)) + [10.0, -20.0, 30.0]).astype(F32)
    lo, hi = xyz.min(0), xyz.max(0)
    for rule in ("old", "new"):
        n = cp.dims(rule, 50.0, lo, hi)
        assert (n == 1).all()
        assert (cp.cells(rule, xyz, lo, 50.0, n) == 0).all()


def test_the_probe_clouds_lose_neighbours_under_the_old_rule():
    """The generators of the GPU tests (tests/test_gpu_cloud_grid_edges.py) build clusters whose lost point changes a result."""
    xyz, info = cp.radius_probe_cloud(0.7, -37.25, clusters=8)
    assert info["lost3"] > 0 and info["lost6"] > 0
    true, old = cp.neighbour_counts(xyz, 0.7, "radius", info["lo"], info["cells"])
    assert (old < true).any()
    fixed = np.zeros(len(xyz), np.int64)
    n = cp.dims("new", 0.7, xyz.min(0), xyz.max(0))
    for i in range(len(xyz)):
        acc = cp.accept(cp.fdist2(xyz[i], xyz), 0.7, "radius")
        fixed[i] = (acc & cp.found("new", xyz[i], xyz, 0.7, xyz.min(0), n)).sum()
    assert np.array_equal(fixed, true)
    xyz, info = cp.knn_probe_cloud(2.3, -1000.3, k=1, span=(200000, 10, 10), clusters=6)
    assert info["wrong"] > 0 and info["lost"] > 0
