"""GPU parity of the re-key pass (k_refine_rekey) in front of the early time-skewed refine launches: every refine stage and the
whole pair stay bit-equal to the oracle, whatever the re-key installs -- the data-term cache only memoises exact values, so a
right prediction saves misses and a wrong one costs misses, never bits."""
import numpy as np
import pytest

from oracle import oracle as orc
from reconstruction_amd import synth

from helpers import diff_report, oracle_stages, refine_options

pytestmark = pytest.mark.gpu

CASES = {  # (the cases of test_gpu_parity.py's time-skew test)
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


def check_refine(ctx, label):
    for name in CASES:
        cfg, rec, fin = stages(name)
        for q in rec:
            if q["stage"] != "refine":
                continue
            k, v = q["level"], q["v"]
            for iters in (q["iters"], q["iters"] - 1):
                want = q["out"] if iters == q["iters"] else orc.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], iters, cfg.ws, q["mg"][v])
                g = ctx.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], iters, cfg.ws, q["mg"][v])
                assert np.array_equal(g, want), diff_report("%s %s L%d v%d iters %d" % (label, name, k, v, iters), g, want)
        res = ctx.match_pair(cfg)
        for v in range(2):
            assert np.array_equal(res.disparity[v], fin["disparity"][v]), "%s %s: pair, view %d" % (label, name, v)


@pytest.mark.parametrize("T,first,until,rows,side", [(4, 4, 22, 0, 0), (4, 1, 22, 16, 0), (2, 2, 22, 8, 0), (3, 4, 22, 1000, 0),
                                                     (4, 2, 10, 33, 0), (3, 6, 40, 12, 0), (2, 9, 1000, 0, 0), (4, 4, 22, 17, 1),
                                                     (4, 4, 0, 0, 0)])
def test_refine_rekey_sweeps_are_bit_identical(ctx, T, first, until, rows, side):
    """Time-skewed launches from sweep `first` (T = 2, 3, 4), each one that starts before sweep `until` preceded by the re-key pass
    -- the nearest-side neighbour (side 0) or the other one (side 1, a deliberately wrong prediction); until = 0: no re-key, the
    early launches miss heavily -- with chunk heights from 4T rows to the whole level: the oracle's result, bit for bit."""
    with refine_options(ctx, refine_skew_from=first, refine_skew_T=T, refine_skew_min_px=0, refine_skew_rows=rows,
                        refine_rekey_until=until, refine_rekey_side=side):
        check_refine(ctx, "T %d from %d rekey until %d side %d rows %d" % (T, first, until, side, rows))
