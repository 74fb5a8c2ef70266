"""The wide-window passes of the cloud filter on the CPU: (1) csrc/win_index.h -- the split of a window candidate into row and
column -- against / and % for every candidate of the windows the passes form (tests/cpp/win_index_check.cpp, plain g++); (2) what
tests/cloud_lattice_fixtures.py claims about its own maps -- island distances, which window radius first bounds the k + 1 nearest of
each satellite (win_clip's bound restated in numpy), the clipped window widths -- so that tests/test_gpu_cloud_filter_wide.py cannot
pass for the wrong reason."""
import os
import subprocess

import numpy as np
import pytest

import cloud_lattice_fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ncx x ncy: the unclipped windows of 80 / 640 / 1280 pixels and the 2560-pixel one on a 3200-row lattice; windows clipped at the left
# side; the whole lattice copy of the 4096 x 3072 benchmark cloud; the narrowest windows; powers of two
SHAPES = [(161, 161), (1281, 1281), (2561, 2561), (5121, 3200), (2540, 2561), (2494, 2561), (3000, 2561), (4048, 2561), (4176, 3152),
          (1, 7), (1, 100000), (2, 9), (3, 11), (2, 1 << 20), (64, 3000), (1024, 4000), (2048, 2561), (4096, 3152), (65536, 300)]
# the first candidate the multiplication alone gets wrong, where it gets any wrong (uint64 replay of the arithmetic: F.bare_split_wrong)
BARE_FIRST = {(2561, 2561): 3329299, (3000, 2561): 6101999, (4176, 3152): 1553471, (2540, 2561): 1701799}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("win_index") / "win_index_check"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-I" + os.path.join(ROOT, "reconstruction_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "win_index_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(*mode):
        r = subprocess.run([str(exe), *mode, *[str(v) for s in SHAPES for v in s]], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = [tuple(int(t) for t in l.split()) for l in r.stdout.splitlines()]
        assert [row[:2] for row in rows] == SHAPES
        return {row[:2]: row[2:] for row in rows}
    return run


def test_window_candidate_split_equals_division_for_every_candidate(checker):
    """row = c / ncx and col = c % ncx for every c < ncx * ncy of every shape."""
    got = checker()
    print({s: v for s, v in got.items() if v != (0, -1)})
    assert all(v == (0, -1) for v in got.values()), {s: v for s, v in got.items() if v != (0, -1)}


def test_the_shapes_tell_the_bare_multiplication_from_the_exact_split(checker):
    """The same program with the correction step taken out -- the multiplication alone, as the passes split candidates before -- is
    caught on the wide shapes, first at the candidates the uint64 replay names; the shapes with ncx^2 ncy <= 2^32 are exact without it."""
    got = checker("bare")
    for s, first in BARE_FIRST.items():
        assert got[s][0] > 0 and got[s][1] == first == F.bare_split_wrong(*s)[1], (s, got[s])
    assert got[(2561, 2561)][0] == 1262
    for s in SHAPES:
        if s[0] * s[0] * s[1] <= 1 << 32:
            assert got[s] == (0, -1), s


# ---- the fixtures' own claims ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(n, k) for n in F.MAPS for k in F.KS], ids=lambda p: "%s-k%d" % p)
def analysed(request):
    name, k = request.param
    m = F.MAPS[name](k)
    P, xs, ys = m.cloud()
    ix = m.index_of(xs, ys)
    rows = {}
    for isl, px in m.islands.items():
        if "_hub" in isl or isl.startswith("patch"):
            continue
        idx = np.array([ix[p] for p in px])
        tau2, first, clear = m.first_radius(P, idx)
        rows[isl] = (px, tau2, first, clear)
    return m, P, rows


def test_rig_and_size(analysed):
    m, P, rows = analysed
    assert np.allclose(m.R @ m.R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(m.R) - 1.0) < 1e-12 and np.abs(m.T).min() > 0
    assert m.f in (3000.0, 10000.0) and 1000 < len(P) < 30000 and np.isfinite(P).all()
    assert max(m.gw, m.gh) > 2700 and min(m.gw, m.gh) > 1400 and m.gw * m.gh * 16 < 70e6      # the lattice copy: wide, ~65 MB
    # a thin sheet: 3-D distances are pixel distances to within 2 % (lateral spacing 1): island distances in pixels are distances in space
    (x0, y0), (x1, y1) = next(iter(rows.values()))[0][0], m.islands[next(n for n in m.islands if n.endswith("_hub"))][0]
    i0, i1 = (m.index_of(*m.cloud()[1:])[p] for p in ((x0, y0), (x1, y1)))
    d3, dp = np.linalg.norm(P[i0].astype(np.float64) - P[i1]), np.hypot(x0 - x1, y0 - y1)
    assert abs(d3 / dp - 1.0) < 0.02, (d3, dp)


def test_every_satellite_is_decided_where_the_map_says(analysed):
    """The first wave radius whose bound (win_clip's, restated) holds the k + 1 nearest of each satellite point, with 2 % to spare on
    both sides: the satellites with a stated radius have it, the lone points have none, and the radii the map claims to cover are there."""
    m, P, rows = analysed
    seen = set()
    for isl, (px, tau2, first, clear) in rows.items():
        assert clear.all() and len(set(first.tolist())) == 1, (isl, first, np.sqrt(tau2))
        r = int(first[0])
        print("%s k %d %-14s %2d points, (k+1)-th nearest at %6.0f pixels: radius %d" % (m.name, m.k, isl, len(px), np.sqrt(tau2.max()), r))
        assert 3 <= len(px) <= m.k or isl.startswith("lone")                       # "fewer than k + 1" on its own
        if isl in m.expect:
            assert r == (m.expect[isl] or 0), (isl, r)
        # no narrower window can decide it: the tile and list passes (24, 40 pixels) cannot either
        assert (tau2 > 1.02 * m.bound2(P[[m.index_of(*m.cloud()[1:])[p] for p in px]], 40)).all(), isl
        seen.add(r)
    assert m.covers <= seen, (m.covers, seen)


def test_all_maps_together_cover_every_wave_radius():
    assert set().union(*(F.MAPS[n](8).covers for n in F.MAPS)) >= {80, 160, 320, 640, 1280, 2560, 5120}


def test_clipped_windows_where_the_bare_multiplication_went_wrong():
    """wide_f3000's satellites beside the left side: at the radius that decides them (1280) their windows are 2540 and 2494 columns wide
    -- past the ~1626 columns up to which the bare multiplication is exact -- the first one clipped at the bottom too, with its near
    neighbours (the hub) at candidate indices beyond the first one the bare multiplication split wrongly; and a 2560-pixel window takes
    the lattice's full width."""
    for k in F.KS:
        m = F.wide_f3000(k)
        ncx, ncy, qrow = m.window(*m.islands["edge_2540"][0], 1280)
        assert (ncx, qrow) == (2540, 1280) and ncy < 1281 + 100 and ncx * ncx * ncy > 1 << 32 and 1626 < ncx < m.gw
        wrong, first = F.bare_split_wrong(ncx, ncy)
        (hx, hy), (sx, sy) = m.islands["e_hub1"][0], m.islands["edge_2540"][0]
        c_hub = (qrow + hy - sy) * ncx + (hx - m.XL + F.WIN_PAD - max(sx - m.XL + F.WIN_PAD - 1280, 0))
        assert wrong > 0 and 0 <= first < c_hub < ncx * ncy, (wrong, first, c_hub)
        ncx, ncy, qrow = m.window(*m.islands["edge_2494"][0], 1280)
        assert ncx == 2494 and ncx * ncx * ncy > 1 << 32 and F.bare_split_wrong(ncx, ncy)[0] > 0
        assert m.window(*m.islands["far_row1100"][0], 2560)[:2] == (m.gw, m.gh)


@pytest.mark.parametrize("k", F.KS)
def test_the_dense_map_overflows_the_lists_of_the_wave_and_workgroup_forms(k):
    """dense_f3000's two satellites, from the gather restated in numpy (WideMap.listed): every point of `over_a` is first bounded at 320
    pixels, where more candidates lie within its bound than the wave form's list (2048) and the workgroup form's (4096) hold, more than
    1024 of them in one wave's quarter -- the histogram narrowing of wave_knn_select in both forms, and k_sor_window_wg's fallback to one
    wave's gather; every point of `fits_b` at 160 pixels with more than 2048 and at most 4096, no quarter above 1024 -- the workgroup form's
    list put together from its quarters.  The third branch behind the selection, the ascending re-sum, no depth map reaches through a
    window: every distance a window accepts is one from the query, at least its distance to the next pixel's ray (~ a lateral spacing) and
    below the bound (< (WR + 1) spacings), so k + 1 of them stay below 2^30 times the smallest -- asserted here with 2^8 to spare; the tie
    cloud of tests/cloud_range_fixtures.py reaches it through the grid search, which shares the code."""
    m = F.dense_f3000(k)
    P, xs, ys = m.cloud()
    ix = m.index_of(xs, ys)
    assert m.gw < 800 and m.gh < 300 and len(P) < 9000
    for isl, radius, over in (("over_a", 320, True), ("fits_b", 160, False)):
        idx = np.array([ix[p] for p in m.islands[isl]])
        tau2, first, clear = m.first_radius(P, idx)
        assert clear.all() and (first == radius).all() and m.expect[isl] == radius and (tau2 > 1.02 * m.bound2(P[idx], 40)).all()
        for i in idx:
            K, quarters = m.listed(P, xs, ys, i, radius)
            print("%s k %d %s point %d: %d candidates within the bound at %d pixels, per wave %s" % (m.name, k, isl, i, K, radius, quarters))
            assert quarters.sum() == K and K > F.WAVE_LIST
            if over:
                assert K > F.WG_LIST and quarters.max() > F.WG_LIST // 4
            else:
                assert K <= F.WG_LIST and quarters.max() <= F.WG_LIST // 4
            d = np.sqrt(((P[i].astype(np.float64) - P.astype(np.float64)) ** 2).sum(1))
            d = np.sort(d[d > 0])[:k]
            assert d.sum() < 2.0 ** 22 * d[0]


def test_the_thick_sheet_sends_more_than_65536_queries_past_the_list_passes():
    """A sample of 64 of its points: for each the (k + 1)-th nearest lies beyond the bound of the 40-pixel window (with 2 % to spare) and within
    that of a wave pass.  Were that true of fewer than 3/4 of all points, a sample like this had a chance of 1e-8; 3/4 of them are more
    than 65536, so the wave passes are skipped whole."""
    m = F.thick_sheet(30)
    P, xs, ys = m.cloud()
    idx = np.random.default_rng(5).choice(len(P), 64, replace=False)
    tau2, first, clear = m.first_radius(P, idx, radii=(24, 40) + F.WAVE_RADII)
    assert 0.75 * len(P) > 65536 and (first >= 80).all() and (tau2 > 1.02 * m.bound2(P[idx], 40)).all()
