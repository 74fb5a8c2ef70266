"""k_constraints.hip at its carry chains, block edges and widest rows: the five integer stages of MatchOneLayer through the C ABI
against tests/constraints_restatement.py (the reference's serial loops, restated from its text) and against the oracle.  Every
comparison is np.array_equal.

What each group is for (tests/constraints_fixtures.py builds the inputs; tests/test_constraints_cpu.py asserts, without a GPU,
that they contain what is said here and that restatement and oracle agree on them):

  uniqueness   k_uniq resolves alive(x) = g(x) || (h(x) && alive(x-1)) per 64-pixel chunk with two ballots and a Kogge-Stone
               prefix, handing a carry bit and p[x-1] from chunk to chunk.  Runs of pixels that live only through p[x-1], 135
               long across two chunk boundaries, from XL on the untouched p[XL-1], of length 1, 2, 63, 64, 65 ending at lanes
               62, 63, 0 and 1 -- alive, and with the head killed so that the whole run must die; pixels kept by p[x+1] at lane
               63 and at XR; margins of 1 to 129 columns and 1 to 5 rows; clamped and empty candidate intervals with
               q[boundary_L+1] read from the next row and from beyond the buffer; for float64 the (int)(p + 0.5) truncation on
               negative values and sums of exactly 2 - 2^-40, 2 and 2 + 2^-40; and q[boundary_L+1] within 2 of +10000, where the
               test against p[x-1] holds exactly when p[x-1] reads NOMATCH, i.e. is NOT alive (k_uniq killed these pixels until
               it was given its serial path for such chunks).
  order        rows of one component of 47..97 pixels (ORD_BIG = 48), spreads of 0, 1 and more than n, components ending at
               list positions 63, 64, 127, 128; then margins of 10432 (the last one under 64 KB of LDS), 10433, 10496 and 16382
               columns against the oracle.
  wide maps    SetBoundary_smooth and both uniqueness instantiations at W = 16384 (256 chunks per row, 38 margin rows).
  blocks       k_smooth and k_median with margins of 255, 256, 257 and 513 columns, one and four pixels from every border,
               and with 2 XR below, at and above W (the slip terms' reads).

Oracle times of the wide order rows, measured on the CPU (one row, serial C): at most 0.2 s per row at 16382 columns for every
kind (the kind with random disparities at every second pixel removes ~3500 pixels there), so no kind is thinned."""
import numpy as np
import pytest

from oracle import oracle as orc

import constraints_fixtures as fx
import constraints_restatement as cr
from helpers import NOMATCH, diff_report

pytestmark = pytest.mark.gpu

UNIQ = fx.uniqueness_fixtures()


def same(name, got, *wants):
    for i, want in enumerate(wants):
        assert got.dtype == want.dtype and np.array_equal(got, want), diff_report("%s (reference %d)" % (name, i), got, want)


# ---------------------------------------------------------------- uniqueness
@pytest.mark.parametrize("name", list(UNIQ))
def test_uniqueness_fixture(ctx, name):
    f = UNIQ[name]
    restated = cr.uniqueness_pass(f.p, f.q, f.own, f.oth)[0]
    oracle = orc.uniqueness_pass(f.p, f.q, f.own, f.oth)
    assert np.array_equal(restated, oracle)
    same(name, ctx.uniqueness_pass(f.p, f.q, f.own, f.oth), restated, oracle)
    if f.chain:      # the three passes, and with the roles swapped
        for a, b, ma, mb in ((f.p, f.q, f.own, f.oth), (f.q, f.p, f.oth, f.own)):
            g0, g1 = ctx.uniqueness(a, b, ma, mb)
            r0, r1 = cr.uniqueness(a, b, ma, mb)
            o0, o1 = orc.uniqueness(a, b, ma, mb)
            same(name + " three passes, first map", g0, r0, o0)
            same(name + " three passes, second map", g1, r1, o1)


@pytest.mark.parametrize("dtype", [np.int16, np.float64], ids=["s16", "f64"])
def test_uniqueness_at_the_widest_row(ctx, dtype):
    m = fx.wide_maps(3, dtype)
    assert m.p.shape == (40, 16384) and m.p.dtype == dtype
    want = orc.uniqueness_pass(m.p, m.q, m.own, m.oth)
    assert 10000 < (want != m.p).sum() < (m.p != NOMATCH).sum() - 10000      # both outcomes in numbers
    same("uniqueness W 16384", ctx.uniqueness_pass(m.p, m.q, m.own, m.oth), want)


# ---------------------------------------------------------------- order
def test_order_narrow_rows(ctx):
    f = fx.order_narrow()
    restated, oracle = cr.order_constraint(f.d, f.own), orc.order_constraint(f.d, f.own)
    assert np.array_equal(restated, oracle)
    same("order narrow", ctx.order_constraint(f.d, f.own), restated, oracle)


@pytest.mark.parametrize("width", fx.ORDER_WIDE_WIDTHS)
def test_order_wide_rows(ctx, width):
    """Against the oracle alone (the dense matrix of a 16382-pixel row is 512 MB).  A refused LDS request surfaces as an
    RsmError of code RSM_E_HIP from order_constraint, not as wrong bits."""
    f = fx.order_wide(width)
    want = orc.order_constraint(f.d, f.own)
    removed = (want != f.d).sum(axis=1)
    assert removed[0] == 0 and removed[1] == 2 and removed[2] >= 250 and removed[3] >= 1000 and removed[4] == 0, removed
    same("order width %d" % width, ctx.order_constraint(f.d, f.own), want)


# ---------------------------------------------------------------- SetBoundary_smooth at the widest row
def test_set_boundary_at_the_widest_row(ctx):
    m = fx.wide_maps(4)
    H, W = m.p.shape
    YL, YR, XL, XR = m.own[:4]
    assert YR - YL + 1 > 32 and (XR - XL) // 64 + 1 == 256
    for y in (9, 22):
        assert (m.mask[y] == 255).all() and (m.p[y] != NOMATCH).sum() == 1
    s1, BLg, BRg = ctx.set_boundary_smooth(m.p, m.mask, m.own, m.oth)
    s2, BLo, BRo = orc.set_boundary_smooth(m.p, m.mask, m.own, m.oth)
    assert s1 == s2 == 0
    # row 9 gets nothing from above or below: the lone pixel's match column x0 + 2 is carried through every chunk to both ends
    x0 = 8000 + 9
    assert BLo[9, XR] == x0 + 2 and BRo[9, XL + 1] == x0 + 2
    sel = np.zeros((H, W), bool)
    sel[YL:YR + 1, XL:XR + 1] = m.mask[YL:YR + 1, XL:XR + 1] == 255
    assert np.array_equal(BLg[sel], BLo[sel]), diff_report("BL", np.where(sel, BLg, 0), np.where(sel, BLo, 0))
    assert np.array_equal(BRg[sel], BRo[sel]), diff_report("BR", np.where(sel, BRg, 0), np.where(sel, BRo, 0))
    assert max(np.abs(BLo[sel].astype(int)).max(), np.abs(BRo[sel].astype(int)).max()) > 16384      # beyond any column, within int16


# ---------------------------------------------------------------- smooth / median at the 256-column blocks
@pytest.mark.parametrize("width", fx.BLOCK_WIDTHS)
def test_smooth_and_median_at_block_edges(ctx, width):
    n = 0
    for c in fx.block_cases(width):
        tag = "width %d margin %s W %d share %.1f" % (width, c.own[:4], c.W, c.share)
        restated, oracle = cr.smooth_constraint(c.d, c.own), orc.smooth_constraint(c.d, c.own)
        assert np.array_equal(restated, oracle), tag
        same("smooth " + tag, ctx.smooth_constraint(c.d, c.own), restated, oracle)
        restated, oracle = cr.median_filter(c.d, c.mask, c.own), orc.median_filter(c.d, c.mask, c.own)
        assert np.array_equal(restated, oracle), tag
        same("median " + tag, ctx.median_filter(c.d, c.mask, c.own), restated, oracle)
        n += 1
    assert n == len(fx.BLOCK_HEIGHTS) * len(fx.BLOCK_INSETS) * 6 * len(fx.BLOCK_SHARES)


def test_median_at_every_window_count(ctx):
    f = fx.median_counts_map()
    k = np.full(f.d.shape, -1)
    restated, oracle = cr.median_filter(f.d, f.mask, f.own, counts=k), orc.median_filter(f.d, f.mask, f.own)
    YL, YR, XL, XR = f.own[:4]
    inside = k[YL:YR + 1, XL:XR + 1]
    centre = f.d[YL:YR + 1, XL:XR + 1] != NOMATCH
    assert {int(v) for v in inside[centre]} == set(range(1, 7)) and {int(v) for v in inside[~centre]} == set(range(0, 6))
    assert np.array_equal(restated, oracle)
    same("median counts", ctx.median_filter(f.d, f.mask, f.own), restated, oracle)
