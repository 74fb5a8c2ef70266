"""GPU parity of the tile kernel (k_refine_tile): the small levels' refine sweeps T per launch on overlapped tiles.  Every refine
stage and the whole pair stay bit-equal to the oracle for every T the kernel has, from any first sweep, with and without the
re-key pass in front, with 0 .. T - 1 leftover sweeps, on interiors smaller than a tile and not a multiple of it, and with an
update list that overflows -- the data-term cache only memoises exact values, so a dropped record costs misses, never bits."""
import contextlib

import numpy as np
import pytest

from oracle import oracle as orc
from reconstruction_amd import synth

from helpers import TILE_DEFAULTS, diff_report, oracle_stages, refine_options

pytestmark = pytest.mark.gpu

# the tile schedule's defaults (csrc/rsm_ctx.h); helpers.refine_options does not know these names
TILE_MAXT = 8   # RF_TILE_MAXT (csrc/rsm_dev.h)
TX, TY = 32, 16  # the tile a workgroup owns (csrc/k_refine_tile.hip)

CASES = {  # (the cases of test_gpu_refine_rekey.py)
    "s512x384_5levels": dict(width=512, height=384, levels=5, radius=3, offset=2, pair=21, mask_l0_width=16,
                             holes=True, occlude=True),
    "s192x128_ellipse": dict(width=192, height=128, levels=3, radius=2, offset=2, pair=3, mask_kind="ellipse",
                             holes=True),
    "s320x160_occluded_neg_r4": dict(width=320, height=160, levels=2, radius=4, offset=3, pair=7, occlude=True,
                                     holes=True, mask_l0_width=120, border_l0=6),
}
_cache = {}


def stages(name):
    if name not in _cache:
        cfg = synth.config_small(**CASES[name])
        _cache[name] = (cfg,) + tuple(oracle_stages(cfg))
    return _cache[name]


@contextlib.contextmanager
def tile_options(ctx, until=22, side=0, **opts):
    """The tile kernel at every level below refine_skew_min_px (the default 1 M: every level of the cases here), with the given
    tile options; everything goes back to the defaults on exit."""
    unknown = set(opts) - set(TILE_DEFAULTS)
    assert not unknown, unknown
    try:
        with refine_options(ctx, refine_rekey_until=until, refine_rekey_side=side):
            for k, v in dict(TILE_DEFAULTS, refine_tile_min_px=0, **opts).items():
                ctx.set_option(k, v)
            yield ctx
    finally:
        for k, v in TILE_DEFAULTS.items():
            ctx.set_option(k, v)


def check_refine(ctx, label):
    for name in CASES:
        cfg, rec, fin = stages(name)
        for q in rec:
            if q["stage"] != "refine":
                continue
            k, v = q["level"], q["v"]
            for iters in (q["iters"], q["iters"] - 1):
                key = ("want", name, k, v, iters)
                if key not in _cache:
                    _cache[key] = q["out"] if iters == q["iters"] else orc.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], iters, cfg.ws, q["mg"][v])
                want = _cache[key]
                g = ctx.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], iters, cfg.ws, q["mg"][v])
                assert np.array_equal(g, want), diff_report("%s %s L%d v%d iters %d" % (label, name, k, v, iters), g, want)
        res = ctx.match_pair(cfg)
        for v in range(2):
            assert np.array_equal(res.disparity[v], fin["disparity"][v]), "%s %s: pair, view %d" % (label, name, v)


def test_the_cases_hold_a_level_smaller_than_a_tile_and_levels_that_are_no_multiple_of_it():
    """What the sweeps below rely on for coverage: among the cases' refine stages there is an interior narrower or shorter than
    one tile, one that is no multiple of the tile in either direction, and one of several tiles both ways (tiles on all four
    margin borders and tiles on none)."""
    small = ragged = many = False
    for name in CASES:
        cfg, rec, fin = stages(name)
        for q in rec:
            if q["stage"] != "refine":
                continue
            YL, YR, XL, XR = q["mg"][q["v"]][:4]
            w, h = XR - XL - 1, YR - YL - 1
            small |= 0 < w < TX or 0 < h < TY
            ragged |= w % TX != 0 and h % TY != 0 and w > TX and h > TY
            many |= w >= 3 * TX and h >= 3 * TY
    assert small and ragged and many


@pytest.mark.parametrize("T,first,until,side,cap", [
    (4, 4, 22, 0, 0),          # the schedule as it ships
    (2, 1, 22, 0, 0), (3, 2, 22, 0, 0), (TILE_MAXT, 4, 22, 0, 0), (4, 9, 22, 0, 0),
    (5, 2, 22, 0, 0), (6, 4, 22, 0, 0), (7, 9, 22, 0, 0),
    (4, 4, 0, 0, 0), (TILE_MAXT, 1, 0, 0, 0),  # no re-key: heavy misses inside the tile kernel
    (3, 4, 22, 1, 0),          # a wrong prediction
    (4, 2, 0, 0, 3),           # heavy misses and an update list of 3 records per shard: nearly every record is dropped
])
def test_refine_tile_sweeps_are_bit_identical(ctx, T, first, until, side, cap):
    """T sweeps per tile launch from sweep `first`, the launches before sweep `until` preceded by the re-key pass (side 1: the wrong
    neighbour; until = 0: none), `iters` and `iters - 1` sweeps (30 (k + 1) sweeps per level: every number of leftover sweeps from
    0 to T - 1 occurs over the levels), every refine stage of the three cases and the whole pair: the oracle's result, bit for bit."""
    with tile_options(ctx, until=until, side=side, refine_tile_T=T, refine_tile_from=first, refine_upd_cap=cap):
        check_refine(ctx, "tile T %d from %d rekey until %d side %d cap %d" % (T, first, until, side, cap))


def test_refine_tile_off_is_the_single_sweep_schedule(ctx):
    """refine_tile_T = 0 and a refine_tile_min_px above every level both leave the small levels on one launch per sweep."""
    with tile_options(ctx, refine_tile_T=0):
        check_refine(ctx, "tile off")
    with tile_options(ctx):
        ctx.set_option("refine_tile_min_px", 2000000000)
        check_refine(ctx, "tile min_px above every level")


@pytest.mark.parametrize("T", [2, 4, TILE_MAXT])
def test_refine_tile_margin_boxes_around_the_tile_size(ctx, T):
    """One refine stage on margin boxes cut out of its own: interiors of a few pixels, one pixel less / exactly / one pixel more
    than one tile and than two tiles, and a box that is no multiple either way -- so single tiles touch all four borders, and
    edge tiles of 1 and of TX - 1 columns (TY - 1 rows) occur.  13 and 14 sweeps from sweep 2: with and without leftovers."""
    name = "s512x384_5levels"
    cfg, rec, fin = stages(name)
    q = [q for q in rec if q["stage"] == "refine" and q["level"] == 3 and q["v"] == 0][0]
    k, v = q["level"], q["v"]
    YL, YR, XL, XR, Wm, Hm = q["mg"][v]
    assert XR - XL - 1 >= 2 * TX + 30 and YR - YL - 1 >= 2 * TY + 20
    x0, y0 = XL + 9, YL + 5
    sizes = [(1, 1), (5, 3), (TX - 1, TY - 1), (TX, TY), (TX + 1, TY + 1), (2 * TX - 1, 2 * TY + 1), (2 * TX, 2 * TY), (2 * TX + 1, 2 * TY - 1),
             (2 * TX + 7, 5), (3, 2 * TY + 9)]
    with tile_options(ctx, refine_tile_T=T, refine_tile_from=2):
        for w, h in sizes:
            box = (y0, y0 + h + 1, x0, x0 + w + 1, Wm, Hm)
            for iters in (13, 14):
                key = ("box", box, iters)
                if key not in _cache:
                    _cache[key] = orc.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], iters, cfg.ws, box)
                g = ctx.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], iters, cfg.ws, box)
                assert np.array_equal(g, _cache[key]), diff_report("T %d interior %d x %d iters %d" % (T, w, h, iters), g, _cache[key])
