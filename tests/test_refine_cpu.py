"""DisparityRefine on the CPU: the numpy restatement of CStereoMatching.cpp:590-680 (tests/refine_restatement.py) against
answers worked out by hand, then against the oracle's C loop bit for bit, on the inputs whose flat windows, fenced zero
islands and disparity jumps make the update's degenerate branches occur in every sweep.  No GPU."""
import numpy as np
import pytest

from oracle import oracle as orc

import refine_restatement as rr
from helpers import bits_equal

N = rr.NOMATCH
WS = 0.03


def one_pixel(dC, dE, dW, dN, dS, xi3, ws=WS, at=None):
    """A 5 x 9 map whose only live pixel with neighbours is (2, 4); xi3 = the costs at iMatch + 0, 1, 2 for at = iMatch
    (every other window costs 0.5, 0.25, 0.125 from its left edge on: a wrong iMatch shows)."""
    H, W = 5, 9
    d = np.full((H, W), N)
    d[2, 4], d[2, 5], d[2, 3], d[1, 4], d[3, 4] = dC, dE, dW, dN, dS
    xi = np.empty((H - 2, W - 2, W - 2))
    xi[:] = 0.5 / 2.0 ** (np.arange(W - 2) % 3)
    if at is not None:
        xi[1, 3, at:at + 3] = xi3
    out, st = rr.sweep(d, xi, ws, (0, H - 1, 0, W - 1, W, H))
    assert st["out_of_row"] == 0
    keep = np.ones((H, W), bool)
    keep[2, 4] = False
    assert bits_equal(out[keep], d[keep]), "only the centre is a live pixel with a neighbour pair"
    return out[2, 4]


def f(x):
    return float(np.float64(x))


def test_flat_own_window_gives_ws_ds_over_ws_not_ds():
    """A flat own window: the three costs are 0.5, index 1, pwp = 0, pdp = 0 (.cpp:640-643): u = (0 * 0 + ws ds) / (0 + ws)."""
    rng = np.random.default_rng(3)
    H, W = 5, 9
    own_img = np.full((H, W, 3), 77, np.uint8)
    oth_img = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    xi = orc.refine_xi_table(own_img, oth_img)
    assert (xi == 0.5).all()
    d = np.full((H, W), N)
    d[2, 4], d[2, 5], d[2, 3], d[1, 4], d[3, 4] = 0.0, 1.0, 1.5, 0.5, 2.5
    out, _ = rr.sweep(d, xi, WS, (0, H - 1, 0, W - 1, W, H))
    wx, wy = orc.exp_neg(0.25), orc.exp_neg(4.0)   # (|1 - 0| - |1.5 - 0|)^2, (|2.5 - 0| - |0.5 - 0|)^2
    ds = (wx * (1.0 + 1.5) + wy * (0.5 + 2.5)) / (2 * (wx + wy))
    want = (0.0 * 0.0 + WS * ds) / (0.0 + WS)
    assert f(out[2, 4]).hex() == want.hex()
    assert want != ds, "the case must tell ws ds / ws from ds"


def test_mode_1_pixel_index_1():
    """North is NOMATCH: mode 1, the east-west mean (.cpp:658); costs 0.3, 0.1, 0.2: index 1, the parabola's vertex."""
    x0, x1, x2 = 0.3, 0.1, 0.2
    got = one_pixel(0.4, 1.0, 3.0, N, 2.0, (x0, x1, x2), at=3)       # iMatch = int(-1.1) + 4 = 3
    pwp = 0.5 * (x0 + x2) - x1
    pdp = 0.4 + 0.5 * (x0 - x2) / (x0 + x2 - 2 * x1)
    want = (pdp * pwp + WS * (1.0 + 3.0) / 2) / (pwp + WS)
    assert f(got).hex() == want.hex()


def test_mode_2_pixel_index_0():
    """West is NOMATCH: mode 2, the north-south mean (.cpp:661); costs 0.1, 0.3, 0.2: index 0, pdp = d - 0.5."""
    x0, x1, x2 = 0.1, 0.3, 0.2
    got = one_pixel(2.0, 1.0, N, 5.0, 2.0, (x0, x1, x2), at=4)       # iMatch = int(0.5) + 4 = 4
    pwp = x1 - x0
    pdp = 2.0 - 0.5
    want = (pdp * pwp + WS * (5.0 + 2.0) / 2) / (pwp + WS)
    assert f(got).hex() == want.hex()


def test_mode_3_pixel_index_2():
    """Four neighbours, costs 0.3, 0.25, 0.1: index 2 through the second test of .cpp:632; the weighted mean of :670."""
    x0, x1, x2 = 0.3, 0.25, 0.1
    got = one_pixel(-1.0, 0.0, -3.0, 1.0, -1.5, (x0, x1, x2), at=2)  # iMatch = int(-2.5) + 4 = 2
    pwp = x1 - x2
    pdp = -1.0 + 0.5
    ex = abs(0.0 - -1.0) - abs(-3.0 - -1.0)
    ey = abs(-1.5 - -1.0) - abs(1.0 - -1.0)
    wx, wy = orc.exp_neg(ex * ex), orc.exp_neg(ey * ey)
    ds = (wx * (0.0 + -3.0) + wy * (1.0 + -1.5)) / (2 * (wx + wy))
    want = (pdp * pwp + WS * ds) / (pwp + WS)
    assert f(got).hex() == want.hex()


def test_isolated_pixel_keeps_its_value():
    """One neighbour missing on each axis: mode 0, .cpp:655."""
    assert one_pixel(1.75, N, 3.0, 2.0, N, (0.1, 0.2, 0.3), at=4) == 1.75
    assert one_pixel(1.75, N, N, N, N, (0.1, 0.2, 0.3), at=4) == 1.75


def test_both_weights_zero_gives_the_plain_average():
    """t >= 1024 on both axes: wx = wy = 0, .cpp:667-668."""
    x0, x1, x2 = 0.1, 0.3, 0.2
    got = one_pixel(0.0, 40.0, 0.0, 0.0, -35.0, (x0, x1, x2), at=3)  # tx = 1600, ty = 1225; iMatch = int(-1.5) + 4 = 3
    assert orc.exp_neg(1600.0) == 0.0 and orc.exp_neg(1225.0) == 0.0
    ds = (40.0 + 0.0 + -35.0 + 0.0) / 4
    want = ((0.0 - 0.5) * (x1 - x0) + WS * ds) / ((x1 - x0) + WS)
    assert f(got).hex() == want.hex()


@pytest.mark.parametrize("d,trunc,floor", [(-0.2, -1, -2), (0.4, -1, -2), (1.6, 0, 0)])
def test_imatch_truncates_toward_zero(d, trunc, floor):
    """int(d - 1.5) (.cpp:625) is C's conversion: toward zero, not floor.  The background costs differ from window to window,
    so the update tells which three windows were read."""
    assert int(d - 1.5) == trunc and int(np.floor(d - 1.5)) == floor
    got = one_pixel(d, 1.0, 0.0, 1.0, 0.0, None)
    xi = 0.5 / 2.0 ** (np.arange(7) % 3)

    def want(i):
        x0, x1, x2 = (float(v) for v in xi[i:i + 3])
        index = int(x0 >= x1)
        if (x0, x1)[index] > x2:
            index = 2
        if index == 0:
            pwp, pdp = x1 - x0, d - 0.5
        elif index == 2:
            pwp, pdp = x1 - x2, d + 0.5
        else:
            pwp, pdp = 0.5 * (x0 + x2) - x1, d + 0.5 * (x0 - x2) / (x0 + x2 - 2 * x1)
        ex = abs(1.0 - d) - abs(0.0 - d)
        w = orc.exp_neg(ex * ex)
        ds = (w * (1.0 + 0.0) + w * (1.0 + 0.0)) / (2 * (w + w))
        return (pdp * pwp + WS * ds) / (pwp + WS)
    assert f(got).hex() == want(trunc + 4).hex()
    if floor != trunc:
        assert want(floor + 4) != want(trunc + 4)


def test_ring_and_nomatch_are_never_written():
    d, i0, i1, own, states, _ = rr.case("flat_c0")
    first, last = states[0], states[-1]
    YL, YR, XL, XR = own[:4]
    ring = np.ones(first.shape, bool)
    ring[YL + 1:YR, XL + 1:XR] = False
    assert bits_equal(last[ring], first[ring])
    assert np.array_equal(last == N, first == N)
    for (ry, rx) in rr.ISLANDS:   # the fenced islands are fixed points: +0.0 in every sweep
        for s in states:
            assert bits_equal(s[ry, rx], np.zeros_like(s[ry, rx]))


@pytest.mark.parametrize("name", list(rr.INPUTS))
def test_cause_floors(name):
    """The inputs' condition, from the restatement alone: in every sweep each of pwp == 0, |a1| <= 2^-300, |a2| <= 2^-300 on at
    least 32 pixels -- anywhere (where scattered NOMATCH pixels send the whole row to the general update) and inside the rows
    the time-skewed kernel runs straight-line, where its guards decide (the c_ columns) --, no window outside its row, no NaN;
    with the jumps also max(tx, ty) > 200 and >= 512."""
    stats = rr.case(name)[5]
    print("\n%s, ws 0.03: pixels per sweep\n%s" % (name, rr.causes_table(stats)))
    assert rr.check_condition(stats) == []
    assert len(stats) == rr.ITERS and all(st["mode12"] >= rr.CAUSE_FLOOR for st in stats)
    if rr.INPUTS[name]["jumps"]:
        assert all(st["t_gt_200"] >= rr.CAUSE_FLOOR and st["t_ge_512"] >= rr.CAUSE_FLOOR and st["c_t200"] >= rr.CAUSE_FLOOR for st in stats)
        assert stats[0]["wsum0"] > 0


@pytest.mark.parametrize("ws", rr.WS_VALUES, ids=lambda w: float(w).hex())
@pytest.mark.parametrize("name", list(rr.INPUTS))
def test_restatement_equals_oracle(name, ws):
    """Every sweep count 0 .. iters: the restatement's map and the oracle's C loop, the same bits (signed zeros, infinities and
    NaN patterns included), after the inputs' condition has been established for this ws."""
    d, i0, i1, own, states, stats = rr.case(name, ws)
    assert rr.check_condition(stats) == []
    assert all(np.isfinite(s).all() for s in states)
    for n in range(rr.ITERS + 1):
        r = bits_equal(states[n], orc.disparity_refine(d, i0, i1, n, ws, own), "%s ws %s after %d sweeps" % (name, float(ws).hex(), n))
        assert r, r
