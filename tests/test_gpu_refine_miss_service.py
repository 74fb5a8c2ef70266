"""The per-wave miss service (rf_serve_misses, csrc/refine_common.h) in every round pattern: a lane per entry while more than 16
entries are left, four lanes per entry for the rest.  With the default prefill no wave of the quick cases sees more than a few
misses, so the lane-per-entry rounds never run there; without it (refine_prefill = 0) sweep 2 fills the lists.  A CPU census on
the oracle's states shows that the fixture holds waves in every class; the GPU tests hold the three kernels that call the
service -- k_refine_sweep, k_refine_tile, k_refine_rekey -- bit-equal to the oracle on those stages."""
import numpy as np
import pytest

from oracle import oracle as orc
from reconstruction_amd import synth

from helpers import TILE_DEFAULTS, diff_report, oracle_stages, refine_options
from refine_cache_replay import simulate, stage_states, wave_misses

RF_PPT = 4  # rows per thread of k_refine_sweep (csrc/rsm_dev.h): a wave takes 64 columns x RF_PPT rows
# the tile schedule's defaults (csrc/rsm_ctx.h); helpers.refine_options does not know these names

CASES = {  # (two of the cases of test_gpu_refine_rekey.py)
    "s192x128_ellipse": dict(width=192, height=128, levels=3, radius=2, offset=2, pair=3, mask_kind="ellipse",
                             holes=True),
    "s320x160_occluded_neg_r4": dict(width=320, height=160, levels=2, radius=4, offset=3, pair=7, occlude=True,
                                     holes=True, mask_l0_width=120, border_l0=6),
}
_cache = {}


def refine_stages():
    """(case, cfg, record, own image, other image) of every refine stage of the cases; the oracle runs once."""
    if "stages" not in _cache:
        out = []
        for name in CASES:
            cfg = synth.config_small(**CASES[name])
            rec, fin = oracle_stages(cfg)
            for q in rec:
                if q["stage"] == "refine":
                    k, v = q["level"], q["v"]
                    out.append((name, cfg, q, fin["imgs"][k][v], fin["imgs"][k][1 - v]))
        _cache["stages"] = out
    return _cache["stages"]


def want(i, iters):
    name, cfg, q, own, oth = refine_stages()[i]
    if (i, iters) not in _cache:
        _cache[(i, iters)] = orc.disparity_refine(q["inp"], own, oth, iters, cfg.ws, q["mg"][q["v"]])
    return _cache[(i, iters)]


def test_without_prefill_the_stages_hold_waves_in_every_round_pattern():
    """Replays the two-way cache through sweeps 0-2 (single sweeps, no prefill) on the oracle's states and counts the misses per
    k_refine_sweep wave: 64 columns from XL + 1, RF_PPT rows from YL + 1.  The stages hold waves with 1-16 misses (quad rounds
    only), 17-64 (one lane round), 65-80 (a lane round, then a quad round) and more than 80 (two or more lane rounds)."""
    classes = np.zeros(4, np.int64)
    for name, cfg, q, own, oth in refine_stages():
        states, live = stage_states(q["inp"], own, oth, cfg.ws, q["mg"][q["v"]], 2)
        per_sweep = {}
        simulate(states, live, 1, 3, "today", 3, prefill=False, on_single=lambda t, miss: per_sweep.__setitem__(t, wave_misses(miss, RF_PPT)))
        assert sorted(per_sweep) == [1, 2]
        for t, n in per_sweep.items():
            c = np.array([((n >= 1) & (n <= 16)).sum(), ((n >= 17) & (n <= 64)).sum(), ((n >= 65) & (n <= 80)).sum(), (n > 80).sum()])
            print("%s L%d v%d sweep %d: waves by misses [0, 1-16, 17-64, 65-80, >80] = %s, max %d" % (name, q["level"], q["v"], t, [int((n == 0).sum())] + c.tolist(), int(n.max())))
            classes += c
    assert (classes > 0).all(), classes


def check(ctx, label):
    for i, (name, cfg, q, own, oth) in enumerate(refine_stages()):
        for iters in (3, 4):
            g = ctx.disparity_refine(q["inp"], own, oth, iters, cfg.ws, q["mg"][q["v"]])
            w = want(i, iters)
            assert np.array_equal(g, w), diff_report("%s %s L%d v%d iters %d" % (label, name, q["level"], q["v"], iters), g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["single", "tile", "skew_rekey"])
def test_long_miss_lists_are_bit_identical(ctx, schedule):
    """3 and 4 sweeps without the prefill, so that sweep 2 meets the long lists: (single) one launch per sweep, k_refine_sweep
    serves them; (tile) k_refine_tile with T = 2 from sweep 1 and no re-key serves them; (skew_rekey) k_refine_skew with T = 2
    from sweep 1 behind the re-key pass, so k_refine_rekey serves them.  The oracle's result, bit for bit."""
    opts = dict(single=dict(refine_skew_from=0),
                tile=dict(refine_rekey_until=0),
                skew_rekey=dict(refine_skew_from=1, refine_skew_T=2, refine_skew_min_px=0, refine_rekey_until=22))[schedule]
    tile = dict(TILE_DEFAULTS, **(dict(refine_tile_T=2, refine_tile_from=1) if schedule == "tile" else dict(refine_tile_T=0)))
    try:
        ctx.set_option("refine_prefill", 0)
        for k, v in tile.items():
            ctx.set_option(k, v)
        with refine_options(ctx, **opts):
            check(ctx, schedule)
    finally:
        ctx.set_option("refine_prefill", 1)
        for k, v in TILE_DEFAULTS.items():
            ctx.set_option(k, v)
