"""DisparityRefine's sweep loop (CStereoMatching.cpp:590-680) restated in vectorised numpy fp64 from the reference's source,
independently of oracle/stereo_oracle.c's loop and of the HIP kernels.  No GPU, no context, nothing imported from the product.

Two things are taken from the oracle, both pinned on their own: the matching cost xi of .cpp:624-629
(`oracle.refine_xi_table`, bit for bit the compiled reference's: test_oracle_golden.py) and the specified exp of the weights
(`oracle.exp_neg_array`: test_oracle_exp_control.py).  Everything else -- the NOMATCH skip, `mode`, `int(dC - 1.5) + x`, `index`,
pwp / pdp with the `pwp == 0 -> pdp = 0` rule, the four update forms, the `wx + wy == 0` average and the ring that is never
written -- is written here, every expression in the source's order, one rounding per operation (numpy fuses nothing).

The xi table holds the windows that lie inside their row, the reference reads past the row's ends without a check (.cpp:628).
`sweep` therefore counts the live pixels whose iMatch or iMatch + 2 leaves [0, W - 3]; a comparison is valid only when that
count is 0 (such a pixel's xi is taken from the clamped column, i.e. it is wrong here).

`causes` names, per sweep, what makes the time-skewed kernel give up a lane's straight-line result (the documented guards,
copied here as numbers): pwp == 0, |a1| <= 2^-300, |a2| <= 2^-300, max(tx, ty) > 200, and max(tx, ty) >= 512 (the exp's
special case; from ~745 on both axes the weights are 0 and `wx + wy == 0` holds, counted as `wsum0`)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc

NOMATCH = -10000.0          # CStereoMatching.h: the invalid disparity
GUARD_SMALL = 2.0 ** -300   # the skewed kernel's guard on |a1| and |a2|
GUARD_T = 200.0             # ... and on max(tx, ty)
T_SPECIAL = 512.0           # the specified exp's special case starts here

# the ws values of the comparisons: the default, 1, the skewed kernel's guard interval's ends and the doubles just outside, and
# two far outside
WS_VALUES = (0.03, 1.0, 2.0 ** -200, float(np.nextafter(2.0 ** -200, 0.0)), 2.0 ** 200, float(np.nextafter(2.0 ** 200, np.inf)),
             1e-70, 1e70)


def exp_neg(t):
    t = np.asarray(t, np.float64)
    return orc.exp_neg_array(t).reshape(t.shape)


def sweep(d, xi, ws, own):
    """One Jacobi sweep (.cpp:594-674) of the fp64 map `d` [H, W].  xi: [H-2, W-2, W-2] as oracle.refine_xi_table gives it.
    own = (YL, YR, XL, XR, ...).  Returns (new map, stats); `d` is left unchanged."""
    d = np.asarray(d, np.float64)
    H, W = d.shape
    ws = np.float64(ws)
    YL, YR, XL, XR = (int(v) for v in own[:4])
    out = d.copy()                                  # what the loop does not write keeps its value (both buffers start equal, .cpp:587)
    ys, xs = slice(YL + 1, YR), slice(XL + 1, XR)   # y = YL+1 .. YR-1, x = XL+1 .. XR-1 (.cpp:595, :611)
    dC = d[ys, xs]
    dE, dW = d[ys, XL + 2:XR + 1], d[ys, XL:XR - 1]
    dN, dS = d[YL:YR - 1, xs], d[YL + 2:YR + 1, xs]
    live = dC != NOMATCH                            # :613
    mode = ((dE != NOMATCH) & (dW != NOMATCH)).astype(np.int64) + ((dS != NOMATCH) & (dN != NOMATCH)).astype(np.int64) * 2  # :620
    Y, X = np.meshgrid(np.arange(YL + 1, YR), np.arange(XL + 1, XR), indexing="ij")
    with np.errstate(all="ignore"):
        iMatch = np.trunc(dC - 1.5).astype(np.int64) + X        # :625, int(): toward zero
        windows = live & (mode != 0)
        out_of_row = int((windows & ((iMatch < 0) | (iMatch + 2 > W - 3))).sum())
        col = [np.clip(iMatch + i, 0, W - 3) for i in range(3)]
        x0, x1, x2 = (xi[Y - 1, X - 1, c] for c in col)         # :626-630
        index = (x0 >= x1).astype(np.int64)                     # :631
        index = np.where(np.where(index == 1, x1, x0) > x2, 2, index)  # :632
        pwp1 = 0.5 * (x0 + x2) - x1                             # :640
        pdp1 = dC + 0.5 * (x0 - x2) / (x0 + x2 - 2 * x1)        # :641
        pdp1 = np.where(pwp1 == 0, 0.0, pdp1)                   # :642-643
        pwp = np.where(index == 0, x1 - x0, np.where(index == 2, x1 - x2, pwp1))   # :636, :646
        pdp = np.where(index == 0, dC - 0.5, np.where(index == 2, dC + 0.5, pdp1))  # :637, :647
        u1 = (pdp * pwp + ws * (dE + dW) / 2) / (pwp + ws)      # :658
        u2 = (pdp * pwp + ws * (dN + dS) / 2) / (pwp + ws)      # :661
        ex = np.abs(dE - dC) - np.abs(dW - dC)
        ey = np.abs(dS - dC) - np.abs(dN - dC)
        tx, ty = ex * ex, ey * ey                               # square_
        wx, wy = exp_neg(tx), exp_neg(ty)                       # :665-666
        a1 = wx * (dE + dW) + wy * (dN + dS)
        ds = np.where(wx + wy == 0, (dE + dW + dS + dN) / 4, a1 / (2 * (wx + wy)))  # :667-670
        a2 = pdp * pwp + ws * ds
        u3 = a2 / (pwp + ws)                                    # :671
        new = np.where(mode == 0, dC, np.where(mode == 1, u1, np.where(mode == 2, u2, u3)))  # :652-672
    out[ys, xs] = np.where(live, new, dC)
    m3 = live & (mode == 3)
    tmax = np.maximum(tx, ty)
    # the rows of a strip that the time-skewed kernel (4 sweeps per launch: 64 lanes from column ((XL + 1 - 3) & ~7) + 58 b, of
    # which it owns 58 from the fourth on) runs straight-line: no live pixel with exactly one neighbour pair among the lanes
    one_pair = windows & (mode != 3)
    common = np.zeros_like(live)
    for x0 in range((XL + 1 - 3) & ~7, XR, 58):
        lanes = slice(max(x0 - (XL + 1), 0), max(x0 + 64 - (XL + 1), 0))
        owned = slice(max(x0 + 3 - (XL + 1), 0), max(x0 + 61 - (XL + 1), 0))
        common[:, owned] = ~one_pair[:, lanes].any(axis=1)[:, None]
    c3 = m3 & common
    stats = dict(live=int(live.sum()), mode0=int((live & (mode == 0)).sum()), mode12=int((windows & (mode != 3)).sum()),
                 mode3=int(m3.sum()), out_of_row=out_of_row,
                 pwp0=int((windows & (pwp == 0)).sum()),
                 a1_small=int((m3 & (np.abs(a1) <= GUARD_SMALL)).sum()),
                 a2_small=int((m3 & (np.abs(a2) <= GUARD_SMALL)).sum()),
                 t_gt_200=int((m3 & (tmax > GUARD_T)).sum()),
                 t_ge_512=int((m3 & (tmax >= T_SPECIAL)).sum()),
                 wsum0=int((m3 & (wx + wy == 0)).sum()),
                 c_rows=int(common.sum()),
                 c_pwp0=int((c3 & (pwp == 0)).sum()),
                 c_a1=int((c3 & (np.abs(a1) <= GUARD_SMALL)).sum()),
                 c_a2=int((c3 & (np.abs(a2) <= GUARD_SMALL)).sum()),
                 c_t200=int((c3 & (tmax > GUARD_T)).sum()),
                 nan=int(np.isnan(out).sum()),
                 max_abs=float(np.abs(out[out != NOMATCH]).max()) if (out != NOMATCH).any() else 0.0)
    return out, stats


def refine(disp, img_own, img_oth, iters, ws, own, xi=None):
    """DisparityRefine on the int16 map `disp` (.cpp:585: convertTo fp64).  Returns (states, stats): states[n] is the map after
    n sweeps (n = 0 .. iters), stats[n - 1] the counts of sweep n."""
    if xi is None:
        xi = orc.refine_xi_table(img_own, img_oth)
    states = [np.asarray(disp, np.int16).astype(np.float64)]
    stats = []
    for _ in range(iters):
        nxt, st = sweep(states[-1], xi, ws, own)
        states.append(nxt)
        stats.append(st)
    return states, stats


def causes(disp, img_own, img_oth, iters, ws, own, xi=None):
    """Per sweep 1 .. iters: the number of live pixels with each reason for which the time-skewed kernel redoes a row."""
    return refine(disp, img_own, img_oth, iters, ws, own, xi)[1]


CAUSE_KEYS = ("pwp0", "a1_small", "a2_small", "t_gt_200", "t_ge_512", "wsum0", "mode12", "c_pwp0", "c_a1", "c_a2", "c_t200",
              "out_of_row", "nan")


def causes_table(stats):
    lines = ["sweep " + " ".join("%8s" % k for k in CAUSE_KEYS)]
    for n, st in enumerate(stats):
        lines.append("%5d " % (n + 1) + " ".join("%8d" % st[k] for k in CAUSE_KEYS))
    return "\n".join(lines)


# ---- the inputs ------------------------------------------------------------------------------------------------------------
H_IN, W_IN, ITERS = 48, 150, 26
# (rows, columns) of the three flat blocks; the second straddles the 58-column strips' border at column 61, the third the one
# at 119
BLOCK_SAT = (slice(5, 19), slice(10, 40))      # 255 in both views
BLOCK_OWN = (slice(21, 35), slice(20, 96))     # 0 in the own view only
BLOCK_OTH = (slice(5, 19), slice(100, 132))    # 0 in the other view only
BLOCK_CHK = (slice(22, 34), slice(100, 140))   # 2 x 2 cells of d = centre +- 1
# islands of d = 0 inside a one-pixel NOMATCH ring, at least one pixel inside their block and two inside the flat windows' area
ISLANDS = ((slice(8, 16), slice(14, 36)), (slice(24, 32), slice(24, 46)))
# A ring makes pixels with one neighbour pair beside it, and a row of a strip that holds one is not a common row of the
# time-skewed kernel -- nor is any row with scattered NOMATCH pixels.  So the random NOMATCH pixels (16 %) lie in the upper
# part only (rows < NOMATCH_ROWS: ~8 % of the margin), the second island inside the first strip's lanes, and a third zero
# region needs no ring at its sides: the rows from ZERO_ROWS on are d = 0 over the whole width, margin columns and last margin
# row included (never written: they fence like a ring), under a full row of NOMATCH; the own view is flat in ZERO_FLAT's columns.
# Its zeros erode from the textured ends by one column per sweep and last beyond sweep 26 in the middle.
NOMATCH_ROWS = 20
ZERO_FENCE_ROW, ZERO_ROWS = 36, 37
ZERO_FLAT = slice(30, 121)
JUMP_COLS = (78, 96)
BAND_COLS = (74, 77)


def build_input(seed=14, shift=0, centre=0, jumps=False, H=H_IN, W=W_IN):
    """The degenerate refine input: returns (disp int16, img_own, img_oth, own).
    shift 0: the other view is the own view, minima near d = 0; shift +-2: the other view is the own one moved by two columns
    (as test_refine_block_edges has it), to go with centre = +-2.  Random d in centre + {-1, 0, 1}, ~8 % NOMATCH, the flat
    blocks, the checkerboard, the fenced islands and the zero rows above.  jumps: the disparity steps of
    test_refine_with_weights_across_the_exps_whole_range in columns 78 .. 95 and a band at 74 .. 76 (so that no window leaves
    its row), inside the own-flat block."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(H, W + 8, 3)).astype(np.uint8)
    img0 = np.ascontiguousarray(base[:, 4:W + 4])
    img1 = np.ascontiguousarray(base[:, 4 - shift:W + 4 - shift])
    img0[BLOCK_SAT] = 255
    img1[BLOCK_SAT] = 255
    img0[BLOCK_OWN] = 0
    img1[BLOCK_OTH] = 0
    img0[ZERO_FENCE_ROW:, ZERO_FLAT] = 0
    d = (centre + rng.integers(-1, 2, size=(H, W))).astype(np.int16)
    yy, xx = np.mgrid[0:H, 0:W]
    chk = np.where(((yy // 2 + xx // 2) & 1) == 0, 1, -1).astype(np.int16)  # E + W and N + S cancel around centre = 0
    d[BLOCK_CHK] = centre + chk[BLOCK_CHK]
    if jumps:
        c0, c1 = JUMP_COLS
        jump = rng.random((H, W))
        incol = (xx >= c0) & (xx < c1)
        up = incol & (jump < 0.10)
        dn = incol & (jump >= 0.10) & (jump < 0.16)
        d[up] += rng.integers(18, 30, size=int(up.sum())).astype(np.int16)      # t around 500 ... 900
        d[dn] -= rng.integers(30, 46, size=int(dn.sum())).astype(np.int16)      # t beyond 1024
        d[:, BAND_COLS[0]:BAND_COLS[1]] += 40                                    # a band far away: both weights 0 along its edges
    d[(rng.random((H, W)) < 0.16) & (yy < NOMATCH_ROWS)] = int(NOMATCH)
    for (ry, rx) in ISLANDS:
        d[ry.start - 1:ry.stop + 1, rx.start - 1:rx.stop + 1] = int(NOMATCH)
        d[ry, rx] = 0
    d[ZERO_FENCE_ROW] = int(NOMATCH)
    d[ZERO_ROWS:] = 0
    own = (3, H - 4, 4, W - 5, W - 8, H - 6)
    return d, img0, img1, own


# name -> build_input's arguments: both inputs, and the second disparity sign on shifted views
INPUTS = {
    "flat_c0": dict(shift=0, centre=0, jumps=False),
    "jumps_c0": dict(shift=0, centre=0, jumps=True),
    "flat_neg2": dict(shift=-2, centre=-2, jumps=False),
    "jumps_pos2": dict(shift=2, centre=2, jumps=True),
}
CAUSE_FLOOR = 32  # pixels per sweep with each of pwp == 0, |a1| <= 2^-300, |a2| <= 2^-300 -- anywhere, and inside common rows

_cache = {}


def case(name, ws=0.03, iters=ITERS):
    """(disp, img_own, img_oth, own, states, stats) of an input of INPUTS, computed once per (name, ws)."""
    key = (name, float(ws), iters)
    if key not in _cache:
        if ("in", name) not in _cache:
            d, i0, i1, own = build_input(**INPUTS[name])
            _cache[("in", name)] = (d, i0, i1, own, orc.refine_xi_table(i0, i1))
        d, i0, i1, own, xi = _cache[("in", name)]
        states, stats = refine(d, i0, i1, iters, ws, own, xi)
        for s in states:
            s.setflags(write=False)
        _cache[key] = (d, i0, i1, own, states, stats)
    return _cache[key]


def check_condition(stats):
    """The inputs' condition: in every sweep each degenerate cause on >= CAUSE_FLOOR pixels, no window out of its row, no
    NaN.  Returns the list of violations (empty: holds)."""
    bad = []
    for n, st in enumerate(stats):
        for k in ("pwp0", "a1_small", "a2_small", "c_pwp0", "c_a1", "c_a2"):
            if st[k] < CAUSE_FLOOR:
                bad.append("sweep %d: %s on %d pixels" % (n + 1, k, st[k]))
    for n, st in enumerate(stats):
        if st["out_of_row"] or st["nan"]:
            bad.append("sweep %d: %d windows out of their row, %d NaN" % (n + 1, st["out_of_row"], st["nan"]))
    return bad
