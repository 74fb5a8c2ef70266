"""The cloud kernels' local plane fit (pcl_plane_from_cov behind k_cloud_normals, k_normals_lattice and k_mls<0|1|2>) on the MI355X
against tests/plane_fit_reference.py: numpy.linalg.eigh of a long-double two-pass covariance and a lstsq polynomial fit, which share
no formula with the kernels, their oracle or their restatement.  Every point with a usable reference is held to its own bound --
float32 rounding plus 4 K times the double rounding times the point's conditioning, K as tests/test_plane_fit_cpu.py measured it on
the CPU references -- with no percentile and no absolute escape; the points left out are counted.  On the lattice fixture the rare
branches are reached (the census of test_plane_fit_cpu.py) and the exact results are asked for exactly: axis planes, the NaN planes of
the restated PCL 1.7.2 (a line, a repeated point, an isotropic covariance: NaN normal, and a NaN point out of MLS), the r0 <= 0
fallback's curvature 0.  Each test prints its worst err / bound per kernel and fixture (profiles/f25_plane_fit_tests.log)."""
import numpy as np
import pytest

import plane_fit_reference as pf
from mls_restatement import mls

pytestmark = pytest.mark.gpu

CAM = np.array([30.0, -20.0, 0.0], np.float32)      # off every axis
NOISY = ("dense", "sparse", "far", "sheet")
_lattice = {}


def report(kernel, fixture, cmp):
    ratios = pf.worst_ratio(cmp)
    for which, ratio in sorted(ratios.items()):
        print("f25 %-18s %-8s %-10s worst err / bound %.4f over %d values" % (kernel, fixture, which, ratio, cmp[which][0].size))
    return ratios


def within(kernel, fixture, cmp):
    ratios = report(kernel, fixture, cmp)
    assert all(r <= 1.0 for r in ratios.values()), (kernel, fixture, ratios)


def dot32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def filter_normals(ctx, fx):
    """k_cloud_normals through the host entry: an outlier removal that removes nothing, then the radius normals."""
    kept, nrm, _ = ctx.filter_cloud(fx["xyz"], 20, 1e9, fx["r"], CAM)
    assert np.array_equal(kept, np.arange(len(fx["xyz"])))
    return nrm


def mls_rows(ctx, fx, order, use_ref):
    gx, gn, gi = ctx.mls_cloud(fx["xyz"], fx["r"], order, fx["ref"] if use_ref else None)
    assert np.array_equal(gi, np.nonzero(fx["emitted"])[0])                # the emitted set: the finite points with 3 neighbours and more
    if use_ref:                                                            # :378-385: no output normal against its input point's
        fin = np.isfinite(fx["ref"][gi, 0]) & np.isfinite(gn[:, 0])
        assert (dot32(gn[fin], fx["ref"][gi][fin]) >= 0).all()
    return pf.scatter(len(fx["xyz"]), gi, gx, gn)


def lattice_restated():
    if not _lattice:
        fx = pf.fixture("lattice")
        _lattice["ref"] = mls(fx["xyz"], fx["r"], (0, 1, 2), fx["ref"])
        _lattice["noref"] = mls(fx["xyz"], fx["r"], (0, 1, 2))
    return _lattice


# ---------------------------------------------------------------- the noisy clouds, generic route
@pytest.mark.parametrize("name", NOISY)
def test_cloud_normals_within_each_points_bound(ctx, name):
    """k_cloud_normals: one-pass covariance, so the bound carries kappa1 -- on the far cloud (x, y ~ 2e4, z ~ 5e4) cnt |c|^2 is 1e11
    times a neighbourhood's own spread, which is where a one-pass covariance goes wrong first."""
    fx = pf.fixture(name)
    nrm = filter_normals(ctx, fx)
    assert np.array_equal(np.isnan(nrm[:, 0]), ~fx["emitted"])
    left_out = int((fx["emitted"] & ~fx["mask"][0]).sum())
    print("f25 %-18s %-8s %d points, %d emitted, %d left out" % ("k_cloud_normals", name, len(nrm), fx["emitted"].sum(), left_out))
    assert left_out <= 0.02 * fx["emitted"].sum()
    within("k_cloud_normals", name, pf.compare_normals(fx, nrm, one_pass=True))
    e = fx["emitted"]
    assert (dot32(nrm[e], CAM[None] - fx["xyz"][e]) >= 0).all()             # turned toward CamCenter


@pytest.mark.parametrize("use_ref", [True, False])
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("name", NOISY)
def test_mls_within_each_points_bound(ctx, name, order, use_ref):
    fx = pf.fixture(name)
    gx, gn = mls_rows(ctx, fx, order, use_ref)
    assert (fx["emitted"] & ~fx["mask"][order]).sum() <= 0.02 * fx["emitted"].sum()
    within("k_mls<%d>%s" % (order, " ref" if use_ref else ""), name, pf.compare_mls(fx, order, gx, gn))


# ---------------------------------------------------------------- the lattice fixture
def test_cloud_normals_on_the_lattice_fixture(ctx):
    fx = pf.fixture("lattice")
    w, xyz = fx["where"], fx["xyz"]
    nrm = filter_normals(ctx, fx)
    no_plane = np.concatenate([w[c] for c in pf.NO_PLANE])
    undecided = np.concatenate([w[c] for c in pf.UNDECIDED])
    want_nan = ~fx["emitted"]
    assert np.array_equal(np.isnan(nrm[:, 3]), want_nan)                   # fewer than 3 neighbours: all four NaN
    want_nan[no_plane] = True                                              # no plane: a NaN normal with a curvature
    rest = np.setdiff1d(np.arange(len(xyz)), undecided)
    assert np.array_equal(np.isnan(nrm[rest, :3]).any(1), want_nan[rest]) and np.array_equal(np.isnan(nrm[rest, :3]).all(1), want_nan[rest])
    assert (nrm[w["cube"], 3] == np.float32(1.0 / 3.0)).all() and (nrm[np.concatenate([w[c] for c in ("line5", "line4", "repeated4")]), 3] == 0).all()
    for name, axis in pf.EXACT_PLANES.items():
        ii = w[name]
        want = np.zeros((len(ii), 3), np.float32)
        want[:, axis] = np.sign(CAM[axis] - xyz[ii, axis])                  # toward the origin, then toward CamCenter: the last turn decides
        assert np.array_equal(nrm[ii, :3], want) and (nrm[ii, 3] == 0).all(), name
    assert (nrm[w["fallback1"], 3] == 0).all()                              # r0 = -5.5e-10 <= 0: computeRoots2's 0, not |r0| / trace
    within("k_cloud_normals", "lattice", pf.compare_normals(fx, nrm, one_pass=True))
    e = fx["emitted"] & ~want_nan
    assert (dot32(nrm[e], CAM[None] - xyz[e]) >= 0).all()


@pytest.mark.parametrize("use_ref", [True, False])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_mls_on_the_lattice_fixture(ctx, order, use_ref):
    fx = pf.fixture("lattice")
    w, xyz = fx["where"], fx["xyz"]
    emit, rx, rn = lattice_restated()["ref" if use_ref else "noref"][order]
    gx, gn = mls_rows(ctx, fx, order, use_ref)
    rest = fx["emitted"].copy()
    rest[np.concatenate([w[c] for c in pf.UNDECIDED])] = False
    # the NaN / finite pattern of the census; a NaN normal comes with a NaN point
    assert np.array_equal(np.isnan(gn[rest]), np.isnan(rn[rest])) and np.array_equal(np.isnan(gx[rest]), np.isnan(rx[rest]))
    no_plane = np.concatenate([w[c] for c in pf.NO_PLANE])
    assert np.isnan(gn[no_plane, :3]).all() and np.isnan(gx[no_plane]).all() and np.isfinite(gn[no_plane, 3]).all()
    assert np.isfinite(gn[np.setdiff1d(np.nonzero(rest)[0], no_plane)]).all()
    for name, axis in pf.EXACT_PLANES.items():
        ii = w[name]
        want = np.zeros((len(ii), 3))
        want[:, axis] = 1.0
        assert np.array_equal(np.abs(gn[ii, :3]), want) and (gn[ii, 3] == 0).all(), (name, "normal")
        assert np.array_equal(gn[ii, :3], rn[ii, :3].astype(np.float64)), (name, "sign")      # exact sums: the restatement's own sign, or the flip's
        assert np.array_equal(gx[ii].astype(np.float32), xyz[ii]), (name, "position")
    kernel = "k_mls<%d>%s" % (order, " ref" if use_ref else "")
    within(kernel, "lattice", pf.compare_mls(fx, order, gx, gn))
    if order == 2:      # rank 5 of 6: the independent (minimum-norm) fit or the plane's projection, whichever way the pivot rounds
        m = np.zeros(len(xyz), bool)
        m[np.concatenate([w[c] for c in pf.RANK_DEFICIENT])] = True
        as_fit, as_plane = pf.compare_mls(fx, 2, gx, gn, mask=m)["pos"], pf.compare_mls(fx, 0, gx, gn, mask=m)["pos"]
        ok_fit = (as_fit[0] <= pf.bound(as_fit[1], as_fit[2], "pos", pf.KERNEL_K)).all(1)
        ok_plane = (as_plane[0] <= pf.bound(as_plane[1], as_plane[2], "pos", pf.KERNEL_K)).all(1)
        print("f25 %-18s lattice  rank-deficient footprint: %d of %d took the plane" % (kernel, ok_plane.sum(), m.sum()))
        assert (ok_fit | ok_plane).all()


# ---------------------------------------------------------------- the pixel-lattice route
@pytest.mark.parametrize("case", [0, 5])
def test_lattice_normals_within_each_points_bound(ctx, case):
    """k_normals_lattice (the window form of the normals on a matched pair's cloud, radius 9) on 1500 sampled points of the
    downloaded records, their neighbourhoods by brute force among all records."""
    from reconstruction_amd import synth
    from test_gpu_cloud_filter import PAIRS_W
    ctx.match_pair(synth.config_small(**PAIRS_W[case]), want_cloud=False)
    cam = (3.0 * case + 1.0, -2.0, 1.0)
    ctx.set_option("filter_normals_window", 40)
    try:
        rec, nrm, _ = ctx.filter_last_cloud_host(100, 1.0, 9.0, cam)
        info = ctx.filter_last_info()
    finally:
        ctx.set_option("filter_normals_window", 8)
    assert info["normals_window"] > 0, info
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], 1)
    q = np.sort(np.random.default_rng(25 + case).choice(len(xyz), min(1500, len(xyz)), replace=False))
    ptr, idx = pf.neighbourhoods(xyz, 9.0, queries=q)
    pl = pf.plane(xyz, ptr, idx)
    emitted = pl["cnt"] >= 3
    assert np.array_equal(np.isnan(nrm[q, 0]), ~emitted)
    fx = dict(pl=pl, mask={0: emitted & pl["usable"]})
    left_out = int((emitted & ~pl["usable"]).sum())
    print("f25 %-18s pair %d   %d records, window %d, %d sampled, %d emitted, %d left out" % ("k_normals_lattice", case, len(xyz), info["normals_window"], len(q),
                                                                                           emitted.sum(), left_out))
    assert emitted.sum() > 100 and left_out <= 0.02 * emitted.sum()       # (pair 0's points lie 12 to 19 apart: few have 3 neighbours within 9)
    within("k_normals_lattice", "pair %d" % case, pf.compare_normals(fx, nrm[q], one_pass=True))
    assert (dot32(nrm[q][emitted], np.asarray(cam, np.float32)[None] - xyz[q][emitted]) >= 0).all()
