"""The cloud filter's wide-window passes on WIDE lattices (csrc/k_filter.hip: wave_passes -- k_filter_win.hip's k_sor_window_wave / k_sor_window_wg over windows
of 80 ... 2560 pixels and the pass that covers the box -- the whole-cloud search over a lattice copy of millions of cells, the hand-over at
65536 queries): the sparse depth maps of tests/cloud_lattice_fixtures.py (margin boxes of ~2700 x 1400 and 1400 x 2700 pixels, a few thousand
points) through rsm_stage_filter_depth_map, which filters a given depth map exactly as rsm_filter_last_cloud filters a matched pair's.
Every map three ways, all points taking part: against the same call with the pixel-window passes off (the generic grid search), against
oracle/cloud_oracle.c (PCL's statistical outlier removal by brute force) and against rsm_filter_cloud on the downloaded cloud -- kept set,
normals and the statistics' bits -- with `filter_wg_max` 0 / 2048 / 1 << 30 and `filter_list` 4 / 23 / 31; and rsm_filter_last_passes must
say that the routes the maps are built for were taken (tests/test_cloud_lattice_cpu.py holds the maps to their claims without a GPU).
One small map more, dense_f3000, the same three ways: more candidates within a window's bound than the lists of the two forms hold.
Also here: csrc/win_index.h -- the candidate split of those windows -- against the device's own division."""
import numpy as np
import pytest

import cloud_lattice_fixtures as F
from oracle import oracle as orc
from test_cloud_lattice_cpu import SHAPES

pytestmark = pytest.mark.gpu

CAM = (40.0, -30.0, 5.0)
NORMAL_RADIUS = 2.5          # lateral spacing 1: a few dozen points of a dense patch, none of a satellite's surroundings
CONFIGS = [(fl, wg) for fl in (4, 23, 31) for wg in (0, 2048, 1 << 30)]
# the tile pass's pinned radius per `filter_list` (the probe would find no window on such maps): 24, which the wave passes alone (4) need in front
# of them; 16 under 31, so that the 24-pixel list pass runs too -- in the wave form, like the 40-pixel one
WINDOW = {4: 24, 23: 24, 31: 16}
_memo = {}


@pytest.mark.parametrize("ncx,ncy", SHAPES)
def test_window_candidate_split_equals_the_devices_division(ctx, ncx, ncy):
    assert ctx.win_index_check(ncx, ncy) == 0


def _filter(ctx, m, window, fl=23, wg=2048):
    ctx.set_option("filter_window", window)
    ctx.set_option("filter_list", fl)
    ctx.set_option("filter_wg_max", wg)
    try:
        xyz, kept, nrm, st = ctx.filter_depth_map(m.disp, m.mask, m.img, m.Q, m.scale, m.R, m.T, m.own, m.k, 1.0, NORMAL_RADIUS, CAM, max_points=m.n + 8)
        info, passes = ctx.filter_last_info(), ctx.filter_last_passes()
    finally:
        ctx.set_option("filter_window", 1)
        ctx.set_option("filter_list", 23)
        ctx.set_option("filter_wg_max", 2048)
    return dict(xyz=xyz, kept=kept, sig=(kept.tobytes(), nrm.tobytes(), (st["mean"], st["stddev"], st["threshold"])), stats=st, info=info, passes=passes)


def _prepare(maker, k):
    m = maker(k)
    P, xs, ys = m.cloud()
    m.n, m.P = len(P), P
    return m, m.index_of(xs, ys)


def _runs(ctx, name, k):
    """Every call of one map (memoised: the coverage test at the end reads the reports of all of them)"""
    if (name, k) not in _memo:
        m, ix = _prepare({**F.MAPS, **F.DENSE_MAPS}[name], k)
        predicted = {}   # wave radius -> satellite points whose k + 1 nearest it is the first to bound
        for isl, px in m.islands.items():
            if "_hub" in isl or isl.startswith("patch"):
                continue
            tau2, first, clear = m.first_radius(m.P, np.array([ix[p] for p in px]))
            assert clear.all()
            for r in first.tolist():
                predicted[r] = predicted.get(r, 0) + 1
        _memo[(name, k)] = dict(m=m, predicted=predicted, generic=_filter(ctx, m, 0), runs={c: _filter(ctx, m, WINDOW[c[0]], *c) for c in CONFIGS})
    return _memo[(name, k)]


def _check_report(run, fl, wg, predicted):
    """The report of one call against the options and the fixture's predictions; returns {radius: pass}"""
    passes = run["passes"]["passes"]
    lead = {4: [], 23: [40], 31: [24, 40]}[fl]   # the list passes that ran in the wave form
    radii = [p["radius"] for p in passes]
    assert radii[:len(lead)] == lead and radii[len(lead):] == list(F.WAVE_RADII[:len(radii) - len(lead)]), radii
    for p in passes:
        assert p["workgroup"] == (p["entered"] <= wg) and 0 <= p["decided"] <= p["entered"] <= 65536
    for a, b in zip(passes, passes[1:]):
        assert b["entered"] == a["entered"] - a["decided"]
    by_radius = {p["radius"]: p for p in passes}
    for r, cnt in predicted.items():
        if r:   # every satellite point is decided by the first pass whose bound holds its neighbours, by none before
            assert r in by_radius and by_radius[r]["decided"] >= cnt, (r, cnt, passes)
    left = passes[-1]["entered"] - passes[-1]["decided"]
    assert left >= predicted.get(0, 0) and run["info"]["undecided"] == left and run["info"]["radius"] == WINDOW[fl]
    return by_radius


@pytest.mark.parametrize("k", F.KS)
@pytest.mark.parametrize("name", list(F.MAPS) + list(F.DENSE_MAPS))
def test_wide_lattice_three_ways(ctx, name, k):
    R = _runs(ctx, name, k)
    m, generic = R["m"], R["generic"]
    xyz = generic["xyz"]
    # the cloud is the one the fixture predicts from (fp64 arithmetic in another order, then the cast: a last float32 bit at most)
    assert xyz.shape == m.P.shape and np.allclose(xyz, m.P, rtol=3e-7, atol=0)
    assert generic["info"]["radius"] == 0 and generic["passes"] == dict(passes=[], ladder=0, whole=0, whole_over_lattice=False)
    # 2. the brute-force restatement: kept set and the statistics' bits
    keep_o, dist_o, stats_o = orc.sor_filter(xyz, k, 1.0)
    assert np.array_equal(generic["kept"], np.nonzero(keep_o)[0]) and generic["sig"][2] == stats_o
    assert 0 < len(generic["kept"]) < m.n
    # 3. rsm_filter_cloud on the downloaded cloud
    kept_h, nrm_h, st_h = ctx.filter_cloud(xyz, k, 1.0, NORMAL_RADIUS, CAM)
    assert (kept_h.tobytes(), nrm_h.tobytes(), (st_h["mean"], st_h["stddev"], st_h["threshold"])) == generic["sig"]
    # 1. every combination of the passes against the generic search, to the bit; and the routes
    for (fl, wg), run in R["runs"].items():
        assert np.array_equal(run["xyz"], xyz)
        assert run["sig"] == generic["sig"], (name, k, fl, wg)
        by_radius = _check_report(run, fl, wg, R["predicted"])
        print("%s k %d filter_list %2d filter_wg_max %10d: %s | ladder %d, whole-cloud search %d%s" % (
            name, k, fl, wg, " ".join("%d:%d/%d%s" % (p["radius"], p["decided"], p["entered"], "w" if p["workgroup"] else "")
                                      for p in run["passes"]["passes"]),
            run["passes"]["ladder"], run["passes"]["whole"], " over the lattice copy" if run["passes"]["whole_over_lattice"] else ""))
        assert set(m.covers) <= set(by_radius)
        assert run["stats"]["exhaustive"] == run["passes"]["whole"]
        if name == "wide_f3000":
            # clipped windows wider than the ~1626 columns up to which the multiplication alone is exact: the satellites beside the left side are
            # decided at 1280 pixels, where their windows are 2540 and 2494 columns of the lattice's 2764 (test_cloud_lattice_cpu.py)
            widths = [m.window(*m.islands[isl][0], 1280)[0] for isl in ("edge_2540", "edge_2494")]
            assert widths == [2540, 2494] and all(1626 < w < m.gw for w in widths)
            assert by_radius[1280]["decided"] >= len(m.islands["edge_2540"]) + len(m.islands["edge_2494"])
        if name == "dense_f3000":
            # more candidates within the bound than the lists hold (test_cloud_lattice_cpu.py counts them): at 160 pixels the workgroup form's
            # list where the wave form's overflows and narrows, at 320 both narrow, the workgroup form after a quarter has overflowed
            assert by_radius[160]["decided"] >= len(m.islands["fits_b"]) and by_radius[320]["decided"] >= len(m.islands["over_a"])
            assert by_radius[320]["workgroup"] == (wg > 0)
        if name == "lone_f3000":
            # the lone points and the lone island: no window bounds their k + 1 nearest; few enough to skip the ladder -- the whole-cloud
            # search reads the lattice copy (4 million cells) as its point array
            assert run["passes"] == dict(passes=run["passes"]["passes"], ladder=0, whole=k, whole_over_lattice=True), run["passes"]
            assert 5120 in by_radius   # they went through every pass, the one that covers the box included


def test_more_than_65536_queries_skip_the_wave_passes_whole(ctx):
    """The thick sheet: > 65536 queries are left behind the list passes, so no pass of 80 pixels or more may run -- the grid ladder takes them
    all.  Routes only: against the same call with the pixel-window passes off."""
    m, _ = _prepare(F.thick_sheet, 30)
    generic = _filter(ctx, m, 0)
    assert len(generic["xyz"]) == m.n > 65536 and 0 < len(generic["kept"]) < m.n
    for fl, wg in ((23, 2048), (4, 1 << 30)):
        run = _filter(ctx, m, 24, fl, wg)
        ps = run["passes"]
        print("thick sheet filter_list %d: %s, ladder %d, whole-cloud search %d" % (fl, ps["passes"], ps["ladder"], ps["whole"]))
        assert run["sig"] == generic["sig"]
        assert [p["radius"] for p in ps["passes"]] == {23: [40], 4: []}[fl]
        assert ps["ladder"] > 65536 and ps["ladder"] == run["info"]["undecided"] and not ps["whole_over_lattice"]


def test_every_wave_radius_decided_queries_in_both_forms(ctx):
    """Over the module: every radius from 80 to 2560 (and the pass that covers the box) decided at least one query as a wave per query and
    as a workgroup per query, and the whole-cloud search ran over the lattice copy."""
    decided, over_lattice = {}, 0
    for name in F.MAPS:
        for k in F.KS:
            for run in _runs(ctx, name, k)["runs"].values():
                for p in run["passes"]["passes"]:
                    decided[(p["radius"], p["workgroup"])] = decided.get((p["radius"], p["workgroup"]), 0) + p["decided"]
                over_lattice += run["passes"]["whole_over_lattice"]
    print("queries decided per (radius, workgroup form):", sorted(decided.items()))
    for r in F.WAVE_RADII:
        assert decided.get((r, False), 0) > 0 and decided.get((r, True), 0) > 0, (r, decided)
    assert over_lattice > 0
