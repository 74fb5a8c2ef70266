"""The per-pair cloud filter (csrc/k_filter.hip) on clouds whose neighbour distances span many octaves, against oracle/cloud_oracle.c:
where a double sum of float32 values rounds, its bits depend on its order, and PCL's order is sequential and ascending (per point)
and by point index (over the cloud).  tests/cloud_range_fixtures.py builds the clouds, tests/test_cloud_filter_range_cpu.py holds
them to their purpose: the far points and the tight cluster make the host refuse the parallel sums over the cloud (the sequential
branch of distance_threshold, its `bad` flag for the point at 1e20), the small cluster, the underflowing points and the tie cloud
make a query's own sum order-dependent -- in the whole-cloud search and in the grid search's selection."""
import numpy as np
import pytest

import cloud_range_fixtures as crf
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

CAM = np.array([30.0, -20.0, 0.0], np.float32)


def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def stats_equal(st, want):
    got = (st["mean"], st["stddev"], st["threshold"])
    return all(same(a, b) for a, b in zip(got, want))


def hexes(v):
    return tuple(float(x).hex() for x in v)


@pytest.mark.parametrize("name", [name for name, _, _ in crf.wide_clouds()])
def test_wide_range_clouds_equal_the_oracle(ctx, name):
    variant = name.split("-")[0]
    xyz, k = next((x, k) for nm, x, k in crf.wide_clouds() if nm == name)
    keep_o, dist_o, stats_o = crf.wide_oracle(name)
    kept, nrm, st = ctx.filter_cloud(xyz, k, 1.0, 2.5, CAM)
    print("%s: library %s, oracle %s; kept %d / %d, exhaustive %d" % (name, hexes((st["mean"], st["stddev"], st["threshold"])), hexes(stats_o), len(kept),
                                                                     int(keep_o.sum()), st["exhaustive"]))
    assert stats_equal(st, stats_o), (st, stats_o)
    assert np.array_equal(kept, np.nonzero(keep_o)[0])
    nrm_o = orc.cloud_normals(xyz[keep_o], 2.5, CAM)
    assert np.array_equal(np.isnan(nrm[:, 0]), np.isnan(nrm_o[:, 0]))
    if variant in ("far1e6", "far1e9", "far1e20"):
        assert st["exhaustive"] > 0
    if variant == "tight_small":
        # where the cluster's k - 3 queries -- the ones whose sums reach from 1e-9 to the sheet -- are decided.  The ladder hands over to
        # the whole-cloud search once at most 48 queries are left: 17 members (k = 20) end there; 97 (k = 100) stay in the ladder until
        # a level's radius reaches the sheet 600 away and the grid search's selection decides them (measured: exhaustive 44 and 0)
        grid = ctx.filter_last_grid()
        reach = float(grid["h"]) * 2.0 ** (grid["levels"] - 1)
        print("   tight_small: %d members, ladder from h = %g over %d levels (last radius %g)" % (k - 3, grid["h"], grid["levels"], reach))
        if k - 3 <= 48:
            assert st["exhaustive"] >= k - 3
        else:
            assert st["exhaustive"] < k - 3 and reach > 590.0


def test_order_dependent_sums_longer_than_the_lists(ctx):
    """k = 4200: the grid search's selection cannot order a sum of more than its list's 2048 values and hands the query on, and the
    whole-cloud search's finish, whose list holds 4096, reads the points again per distinct value."""
    xyz, k = crf.long_sum_cloud(), crf.LONG_K
    keep_o, dist_o, stats_o = orc.sor_filter(xyz, k, 1.0)
    members = range(crf.WIDE_AT, crf.WIDE_AT + 30)
    assert not any(crf.sum_is_order_free(crf.knn_roots(xyz, i, k)) for i in members)
    kept, nrm, st = ctx.filter_cloud(xyz, k, 1.0, 2.5, CAM)
    print("long sums: library %s, oracle %s; kept %d / %d, exhaustive %d" % (hexes((st["mean"], st["stddev"], st["threshold"])), hexes(stats_o), len(kept),
                                                                             int(keep_o.sum()), st["exhaustive"]))
    assert st["exhaustive"] >= len(members)
    assert stats_equal(st, stats_o), (st, stats_o)
    assert np.array_equal(kept, np.nonzero(keep_o)[0])


def test_tie_cloud_gives_the_ascending_sum_every_time(ctx):
    """n = k + 1: every query ends in the whole-cloud search, whose slices' partial sums meet in the order the workgroups retire."""
    xyz = crf.tie_cloud()
    keep_o, dist_o, stats_o = orc.sor_filter(xyz, crf.TIE_K, 1.0)
    assert float(dist_o[0]) == crf.TIE_DIST0
    seen = []
    for rep in range(20):
        kept, nrm, st = ctx.filter_cloud(xyz, crf.TIE_K, 1.0, 2.5, (0.0, 0.0, 5.0))
        assert st["exhaustive"] == len(xyz)
        seen.append((hexes((st["mean"], st["stddev"], st["threshold"])), kept.tobytes()))
    print("tie cloud, 20 calls: %d distinct results; oracle %s, seen %s" % (len(set(seen)), hexes(stats_o), sorted(set(s[0] for s in seen))))
    assert all(s == (hexes(stats_o), np.nonzero(keep_o)[0].astype(np.int32).tobytes()) for s in seen)


def test_tie_motif_in_the_grid_search(ctx):
    """The tie cloud beside a sheet 600 away, k = 8, the ladder pinned to start at h = 2: the origin's query is decided by the grid
    search's selection (k_sor_knn / wave_knn) on the first level, the motif's other points there or on the second (h = 4),
    which runs because the sheet's outliers leave more than the 48 queries at which the ladder hands over to the whole-cloud
    search.  From the second level on the ladder sees what it sees for the sheet alone, so the same queries reach the whole-cloud
    search as for the sheet alone: none of the motif's."""
    F32 = np.float32
    h, k = F32(2.0), crf.TIE_K
    tie, sheet = crf.tie_cloud(), crf.surface_cloud(3000, 3)
    xyz = np.concatenate([tie, sheet])
    fin = sheet[np.isfinite(sheet).all(1)]
    within = lambda p, pts, r: int((crf.dist2_f32(p, pts) <= F32(r * r)).sum())
    assert within(tie[0], tie, h) == k + 1 and all(within(p, tie, 2 * h) == k + 1 for p in tie)
    left = sum(within(p, fin, h) < k + 1 for p in fin)
    assert left > 48 + len(tie), left
    ctx.set_option("filter_ladder_h", int(h.view(np.int32)))
    try:
        _, _, st_s = ctx.filter_cloud(sheet, k, 1.0, 2.5, CAM)
        kept, nrm, st = ctx.filter_cloud(xyz, k, 1.0, 2.5, CAM)
        grid = ctx.filter_last_grid()
    finally:
        ctx.set_option("filter_ladder_h", 0)
    keep_o, dist_o, stats_o = orc.sor_filter(xyz, k, 1.0)
    print("tie motif in the grid: library %s, oracle %s; exhaustive %d (sheet alone %d), first level undecided %d of the sheet"
          % (hexes((st["mean"], st["stddev"], st["threshold"])), hexes(stats_o), st["exhaustive"], st_s["exhaustive"], left))
    assert float(dist_o[0]) == crf.TIE_DIST0
    assert grid["h"] == h and grid["levels"] >= 2
    assert st["exhaustive"] == st_s["exhaustive"]
    assert stats_equal(st, stats_o), (st, stats_o)
    assert np.array_equal(kept, np.nonzero(keep_o)[0])
