"""The cloud searches at the cell boundaries of their grid (csrc/cloud_grid.h) on the MI355X, against brute force: the MLS
(tests/mls_restatement.py), the filter's radius normals and its k-nearest ladder (oracle/cloud_oracle.c), on the probe clouds of
tests/cloud_probes.py -- clusters whose accepted neighbour a float cell rule puts two cells away, sized so that losing it changes
the result -- at the radii 2.5, 8, 2.3, 0.7 and 0.1, far from and near the origin, on negative coordinates, up to the 2^20-cell
cap, past it, and with a radius wider than the cloud."""
import numpy as np
import pytest
import torch

import cloud_probes as cp
from mls_restatement import mls
from oracle import oracle as orc
from test_gpu_mls import check_against

pytestmark = pytest.mark.gpu

F32 = np.float32
RADIUS_PROBES = [(2.5, -37.25), (8.0, -37.25), (2.3, -1000.3), (0.7, -37.25), (0.1, -(1e5 + 0.3))]
_clouds = {}


def probe(r, o, far=None):
    key = (r, o, far)
    if key not in _clouds:
        xyz, info = cp.radius_probe_cloud(r, o, clusters=40, far=far, expect_loss=far is None or far > o)
        print("probe r %g origin %g far %s: %d points, %d pairs, the float rule loses %d neighbours (%d counts cross 3, %d cross 6); "
              "cells %s" % (r, o, far, len(xyz), info["pairs"], info["lost"], info["lost3"], info["lost6"], [int(c) for c in info["cells"]]))
        _clouds[key] = (xyz, info, mls(xyz, r, (0, 1, 2)))
    return _clouds[key]


def _mls_both_entries(ctx, xyz, r, order):
    """rsm_mls_cloud (host) and rsm_mls_cloud_device on the same points: the same bits."""
    hx, hn, hi = ctx.mls_cloud(xyz, r, order)
    n = len(xyz)
    rec = np.zeros((n, 4), F32)
    rec[:, :3] = xyz
    d_rec = torch.from_numpy(rec).cuda()
    ox = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    on = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    oi = torch.empty(n, dtype=torch.int32, device="cuda")
    m = ctx.mls_cloud_device(d_rec.data_ptr(), n, None, ox.data_ptr(), on.data_ptr(), oi.data_ptr(), r, order)
    assert m == len(hi)
    assert np.array_equal(oi[:m].cpu().numpy(), hi)
    assert np.array_equal(ox[:m].cpu().numpy(), hx, equal_nan=True) and np.array_equal(on[:m].cpu().numpy(), hn, equal_nan=True)
    return hx, hn, hi


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("r,o", RADIUS_PROBES)
def test_mls_keeps_neighbours_across_cell_boundaries(ctx, r, o, order):
    xyz, info, res = probe(r, o)
    emit, rx, rn = res[order]
    gx, gn, gi = _mls_both_entries(ctx, xyz, r, order)
    missing = sorted(set(np.nonzero(emit)[0].tolist()) - set(gi.tolist()))
    assert not missing, ("points without their MLS output", len(missing), missing[:8])
    check_against(gx, gn, gi, emit, rx, rn)


@pytest.mark.parametrize("r,o", RADIUS_PROBES)
def test_filter_normals_keep_neighbours_across_cell_boundaries(ctx, r, o):
    xyz, info, _ = probe(r, o)
    cam = np.array([3.0, -2.0, 1.0], F32) + F32(o)
    kept, nrm, st = ctx.filter_cloud(xyz, 3, 1e30, r, cam)      # (a huge std_mul: SOR keeps every point)
    assert np.array_equal(kept, np.arange(len(xyz)))
    nrm_o = orc.cloud_normals(xyz, r, cam)
    nan_o = np.isnan(nrm_o[:, 0])
    assert np.array_equal(np.isnan(nrm[:, 0]), nan_o), ("NaN pattern", int((np.isnan(nrm[:, 0]) != nan_o).sum()))
    ok = ~nan_o
    assert np.abs(nrm[ok] - nrm_o[ok]).max() < 1e-6


# (first level's search radius, grid origin, box in cells, table kind): the ladder's three forms of k_sor_knn
LADDER = [(2.3, -37.25, (60, 24, 24), 1), (2.3, -1000.3, (200000, 10, 10), 2), (2.3, -37.25, (400, 300, 300), 0)]


@pytest.mark.parametrize("h,o,span,kind", LADDER)
def test_sor_ladder_keeps_neighbours_across_cell_boundaries(ctx, h, o, span, kind):
    """k = 1 and the first level pinned ("filter_ladder_h") to the probes' radius: the level decides p with q -- its nearest point,
    accepted, two float cells away -- or, without q, with a farther point within h.  The kept set, the per-point mean distances'
    mean, stddev and threshold: bit-exact against brute force."""
    k = 1
    xyz, info = cp.knn_probe_cloud(h, o, k=k, span=span)
    keep_o, dist_o, (mean_o, std_o, thr_o) = orc.sor_filter(xyz, k, 1.0)
    ctx.set_option("filter_ladder_h", int(F32(h).view(np.int32)))
    try:
        kept, nrm, st = ctx.filter_cloud(xyz, k, 1.0, 2.5, (0.0, 0.0, 0.0))
        grid = ctx.filter_last_grid()
    finally:
        ctx.set_option("filter_ladder_h", 0)
    # the level as the library built it: its radius, origin, cells and table kind
    assert grid["h"] == F32(h) and grid["kind0"] == kind and kind in grid["kinds"], grid
    assert np.array_equal(grid["origin"], xyz.min(0)), grid
    hi = xyz.max(0)
    lost = cp.knn_route_losses(xyz, grid["h"], k, grid["origin"], cp.dims("old", grid["h"], grid["origin"], hi))
    print("ladder kind %d: %d points, %d clusters, cells %s; the float rule loses %d neighbours, decides %d queries wrongly"
          % (kind, len(xyz), info["clusters"], grid["cells"], lost["lost"], lost["wrong"]))
    assert lost["wrong"] > 0
    assert (st["mean"], st["stddev"], st["threshold"]) == (mean_o, std_o, thr_o)
    assert np.array_equal(kept, np.nonzero(keep_o)[0])
    assert grid["cells"] == cp.dims("new", grid["h"], grid["origin"], hi).tolist(), grid     # (the restatement's cell count)


def test_pinned_ladder_start_gives_the_same_bits(ctx):
    """The option changes the route only: the filter of the probe cloud with the ladder's first level at the sample's estimate,
    pinned fine and pinned coarse, bit for bit."""
    xyz, _ = cp.knn_probe_cloud(2.3, -1000.3, k=1, span=(200000, 10, 10))
    outs = []
    try:
        for h in (0.0, 0.5, 2.3, 40.0):
            ctx.set_option("filter_ladder_h", int(F32(h).view(np.int32)))
            kept, nrm, st = ctx.filter_cloud(xyz, 5, 1.0, 2.5, (1.0, 2.0, 3.0))
            g = ctx.filter_last_grid()
            assert h == 0.0 or g["h"] == F32(h)
            outs.append((kept.tobytes(), nrm.tobytes(), st["mean"], st["stddev"], st["threshold"]))
    finally:
        ctx.set_option("filter_ladder_h", 0)
    assert all(x == outs[0] for x in outs[1:])
    from reconstruction_amd import RsmError
    for bad in (-1, 0x7f800000, 0x7fc00000, 1 << 40):
        with pytest.raises(RsmError):
            ctx.set_option("filter_ladder_h", bad)


@pytest.mark.parametrize("where", ["below", "above"])
def test_clamped_grid_past_the_cell_cap(ctx, where):
    """A far anchor point stretches the box to ~1.4e7 cells on x: the grid stops at 2^20 cells.  Below the cloud, every probe
    point clamps into the last cell; above it, the probes sit in the first cells and the anchor clamps.  MLS and filter normals
    against brute force."""
    r, o = 0.7, -37.25
    far = o - 1e7 if where == "below" else o + 1e7
    xyz, info, res = probe(r, o, far=far)
    assert info["cells"][0] == cp.CAP
    for order in (0, 2):
        emit, rx, rn = res[order]
        gx, gn, gi = _mls_both_entries(ctx, xyz, r, order)
        check_against(gx, gn, gi, emit, rx, rn)
    cam = np.array([0.0, 0.0, 0.0], F32)
    kept, nrm, _ = ctx.filter_cloud(xyz, 3, 1e30, r, cam)
    assert np.array_equal(kept, np.arange(len(xyz)))
    nrm_o = orc.cloud_normals(xyz, r, cam)
    assert np.array_equal(np.isnan(nrm[:, 0]), np.isnan(nrm_o[:, 0]))
    ok = ~np.isnan(nrm_o[:, 0])
    assert np.abs(nrm[ok] - nrm_o[ok]).max() < 1e-6


def test_radius_wider_than_the_cloud(ctx):
    """One cell per axis: every point is every query's candidate (MLS, normals, and the ladder pinned to one cell)."""
    rng = np.random.default_rng(5)
    xyz = (rng.normal(0, 1.0, (300, 3)) * [3.0, 2.0, 0.3] + [-40.0, 25.0, 500.0]).astype(F32)
    r = 50.0
    assert (cp.dims("new", r, xyz.min(0), xyz.max(0)) == 1).all()
    res = mls(xyz, r, (0, 1, 2))
    for order in (0, 1, 2):
        emit, rx, rn = res[order]
        assert emit.all()
        gx, gn, gi = _mls_both_entries(ctx, xyz, r, order)
        check_against(gx, gn, gi, emit, rx, rn)
    cam = np.array([0.0, 0.0, 0.0], F32)
    keep_o, _, (mean_o, std_o, thr_o) = orc.sor_filter(xyz, 10, 1.0)
    ctx.set_option("filter_ladder_h", int(F32(r).view(np.int32)))
    try:
        kept, nrm, st = ctx.filter_cloud(xyz, 10, 1.0, r, cam)
        grid = ctx.filter_last_grid()
    finally:
        ctx.set_option("filter_ladder_h", 0)
    assert grid["cells"] == [1, 1, 1] and grid["kind0"] == 1 and grid["levels"] == 1, grid
    assert (st["mean"], st["stddev"], st["threshold"]) == (mean_o, std_o, thr_o)
    assert np.array_equal(kept, np.nonzero(keep_o)[0])
    nrm_o = orc.cloud_normals(xyz[keep_o], r, cam)
    assert not np.isnan(nrm_o[:, 0]).any() and np.abs(nrm - nrm_o).max() < 1e-6
