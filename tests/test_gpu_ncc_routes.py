"""The NCC matcher's row routing at its thresholds, against the oracle bit for bit and against its restatement row by row.

The initial match is split among four kernels (k_match.hip: the band kernel k_ncc_dot4, k_ncc_wide, the int8 row GEMM
k_ncc_rowgemm, the sliding sums k_ncc_slide) by per-row counts; a pixel that no kernel takes stays NOMATCH, one that two
take is matched twice.  Every case of tests/ncc_routes.py runs through rsm_stage_initial_match under several option sets
(wide_rows 0-3, ncc_mid 0 / 8 / 100 / 160, ncc_slide_max 0 / 512 / a case's widest / 1 << 20): the disparities must be the
oracle's int16 bits, and the routing witness (rsm_stage_last_ncc_routes) must be the restated routing of every row.

Threshold table (both sides of each are reached; test_every_side_of_the_threshold_table_was_reached):
  interval vs NCC_WIDE in a row below RG_MID_MIN mid pixels      160 / 161 candidates
  interval vs ncc_mid in a mid row                               ncc_mid / ncc_mid + 1: each radius's default (R >= 3), 8, 160
  mid pixels vs RG_MID_MIN                                       511 / 512
  wide pixels vs RG_MIN                                          47 / 48
  wide pixels vs RG_SLIDE_MIN                                    1023 / 1024
  widest interval vs ncc_slide_max                               equal / + 1 at 512 and at another value; the value 0
  row GEMM candidate chunks (RG_CC)                              widest 512, 513, 1024, 1025
  sliding-sum plane split (pmax of a workgroup)                  384 / 385, 768 / 769 planes
  listed rows vs RG_SLOTS                                        > 512 GEMM rows, > 512 sliding-sum rows
  worklist vs k_ncc_wide's 8192 workgroups                       8192 / 8193 entries
  tiles (dot4 256, GEMM 64, slide 128 - 2R pixels)               a wide pixel first and last in a tile; XL odd
  image-edge clip                                                a band from column 0 / to column W-1, clipped to 160 / 161
plus: radii 1-7 each take the mid route and the automatic sliding-sum route."""
import numpy as np
import pytest

import ncc_routes as nr
from helpers import diff_report, oracle_stages
from oracle import oracle as orc
from reconstruction_amd import synth

pytestmark = pytest.mark.gpu

CASES = nr.cases()
_oracle_cache = {}
_sides = {}        # (case name, options) -> sides reached, from the witness


def _key(o):
    return tuple(sorted(o.items()))


def _oracle(c):
    if c.name not in _oracle_cache:
        if c.parent is None:
            d = orc.lowest_level_initial_match(c.img_own, c.img_oth, c.mask_own, c.mask_oth, c.r, c.own, c.oth)
        else:
            d = orc.high_level_initial_match(c.img_own, c.img_oth, c.mask_own, c.mask_oth, c.r, c.offset, c.own, c.oth,
                                             c.parent)
        _oracle_cache[c.name] = d
    return _oracle_cache[c.name]


def _set(ctx, o):
    ctx.set_option("wide_rows", o["wide_rows"])
    ctx.set_option("ncc_mid", o["ncc_mid"])
    ctx.set_option("ncc_slide_max", o["ncc_slide_max"])


def _reset(ctx):
    _set(ctx, nr.options())


def witness_mismatch(tag, wit, rt):
    """'' when the library's witness is the restated routing, else a report of the first differing rows"""
    msg = []
    for k in ("wide", "mid", "widest", "route"):
        bad = np.nonzero(wit[k] != rt[k])[0]
        if bad.size:
            msg.append("%s: %s differs in %d rows, first %s: got %s want %s" % (tag, k, bad.size, bad[:6].tolist(),
                                                                                  wit[k][bad[:6]].tolist(), rt[k][bad[:6]].tolist()))
    if wit["worklist"] != rt["worklist"]:
        msg.append("%s: worklist %d want %d" % (tag, wit["worklist"], rt["worklist"]))
    return "\n".join(msg)


def run_case(ctx, c, o):
    """one stage call under options o: (disparities, witness)"""
    _set(ctx, o)
    try:
        got = ctx.initial_match(c.img_own, c.img_oth, c.mask_own, c.mask_oth, c.r, c.offset, c.own, c.oth, c.parent)
        wit = ctx.last_ncc_routes(c.H)
    finally:
        _reset(ctx)
    return got, wit


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_initial_match_routes_at_the_thresholds(ctx, case):
    want = _oracle(case)
    assert (want != nr.NOMATCH).sum() > 0
    bits, routes = [], []
    for o in case.opt_sets:
        tag = "%s %s" % (case.name, ",".join("%s=%d" % kv for kv in _key(o)))
        got, wit = run_case(ctx, case, o)
        rt = case.route(o)
        if not np.array_equal(got, want):
            bits.append(diff_report(tag, got, want))
        m = witness_mismatch(tag, wit, rt)
        if m:
            routes.append(m)
        else:
            _sides[(case.name, _key(o))] = nr.sides(case, rt, wit)
        if case.kind != "noise":
            assert wit["ties"] > 0, (tag, "no pixel reached the reference-order re-evaluation")
    assert not bits, "\n".join(bits[:8])
    assert not routes, "\n".join(routes[:8])


def test_every_side_of_the_threshold_table_was_reached(ctx):
    """From the witnesses of the whole case set (runs the cases this session has not run yet)."""
    got = set()
    for c in CASES:
        for o in c.opt_sets:
            k = (c.name, _key(o))
            if k not in _sides:
                _, wit = run_case(ctx, c, o)
                rt = c.route(o)
                assert not witness_mismatch(c.name, wit, rt), witness_mismatch(c.name, wit, rt)
                _sides[k] = nr.sides(c, rt, wit)
            got |= _sides[k]
    missing = nr.required_sides() - got
    assert not missing, sorted(missing, key=str)


def test_witness_needs_a_stage_call_and_the_same_height(ctx):
    from reconstruction_amd import RsmError
    c = CASES[0]
    run_case(ctx, c, nr.options())
    with pytest.raises(RsmError):
        ctx.last_ncc_routes(c.H + 1)


# ---------------------------------------------------------------- whole pairs
# 2176 x 48, two levels, 7x7 windows (ncc_mid 96): the lowest level (1088 x 24) has rows of ~1076 pixels that each scan ~1077
# candidates -- mid rows, the int8 row GEMM by default, the sliding sums with ncc_slide_max 1 << 20; at the top level the rows
# below an empty parent row scan the whole margin (~2160 candidates).  The oracle's pair costs ~15 s of 8 CPU threads.
PAIR = dict(width=2176, height=48, pyr_levels=2, radius=3, mask_kind="rect", mask_l0_width=1080, border_l0=2)
PAIR_OPTS = [dict(), dict(wide_rows=1), dict(wide_rows=2), dict(wide_rows=3), dict(ncc_mid=8), dict(ncc_mid=100),
             dict(ncc_mid=160), dict(ncc_slide_max=0), dict(ncc_slide_max=1 << 20)]


def test_whole_pair_under_every_option_set(ctx):
    pair = 0
    cfg = synth.make_pair(pair=pair, name="routes_pair%d" % pair, **PAIR)
    ref = orc.match_pair(cfg)
    assert ref["status"] == 0
    rec, fin = oracle_stages(cfg, max_levels=1)       # the lowest level's recorded stage inputs
    fails, taken = [], {}
    for o in map(lambda d: nr.options(**d), PAIR_OPTS):
        tag = "pair%d %s" % (pair, ",".join("%s=%d" % kv for kv in _key(o)))
        _set(ctx, o)
        try:
            res = ctx.match_pair(cfg)
        finally:
            _reset(ctx)
        for v in range(2):
            if not np.array_equal(res.disparity[v], ref["disparity"][v]):
                fails.append(diff_report(tag + " d%d" % v, res.disparity[v], ref["disparity"][v]))
        if res.n_points != ref["n_points"] or not np.array_equal(res.bgr, ref["bgr"]) or \
                not np.array_equal(res.xyz, ref["xyz"], equal_nan=True):
            fails.append("%s: cloud differs (%d / %d points)" % (tag, res.n_points, ref["n_points"]))
        # the lowest level replayed through the stage entry, with the witness
        for q in rec:
            if q["stage"] != "initial":
                continue
            v = q["v"]
            c = nr.Case("pair%d_v%d" % (pair, v), cfg.radius, fin["imgs"][0][v], fin["imgs"][0][1 - v], fin["msks"][0][v],
                        fin["msks"][0][1 - v], None, cfg.offset)
            assert c.own == tuple(q["mg"][v]) and c.oth == tuple(q["mg"][1 - v])
            got, wit = run_case(ctx, c, o)
            if not np.array_equal(got, q["out"]):
                fails.append(diff_report(tag + " replay v%d" % v, got, q["out"]))
            rt = c.route(o)
            m = witness_mismatch(tag + " replay v%d" % v, wit, rt)
            if m:
                fails.append(m)
            mid_rows = (rt["wide_from"] < nr.NCC_WIDE) & (rt["route"] >= nr.ROUTE_GEMM)
            taken.setdefault(_key(o), set()).update(set(wit["route"].tolist()) | ({"mid"} if mid_rows.any() else set()))
    assert not fails, "\n".join(fails[:8])
    assert {"mid", nr.ROUTE_GEMM} <= taken[_key(nr.options())], taken[_key(nr.options())]
    assert nr.ROUTE_SLIDE in taken[_key(nr.options(ncc_slide_max=1 << 20))]
