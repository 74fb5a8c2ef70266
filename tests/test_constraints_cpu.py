"""tests/constraints_restatement.py against the oracle and the reference's goldens, and tests/constraints_fixtures.py against
what it is built to contain (no GPU).

The GPU tests of tests/test_gpu_constraint_chains.py hold k_constraints.hip to the restatement and to the oracle on these
fixtures; here the restatement -- the reference's serial loops, dense matrix and scatter, sharing no code with oracle/ -- is
held to the oracle on the same inputs, to the random maps of test_gpu_parity.test_random_inputs_constraint_stages and to what
the compiled reference returned (tests/golden/), and every condition a fixture exists for is asserted from the restatement's
class maps and row statistics."""
import os

import numpy as np
import pytest

from oracle import oracle as orc

import constraints_fixtures as fx
import constraints_restatement as cr
from helpers import NOMATCH, diff_report

GOLD = os.path.join(os.path.dirname(__file__), "golden")
UNIQ = fx.uniqueness_fixtures()
_classes = {}


def classes(name):
    """(new p, cls, run) of one restated pass over a uniqueness fixture, computed once."""
    if name not in _classes:
        f = UNIQ[name]
        _classes[name] = cr.uniqueness_pass(f.p, f.q, f.own, f.oth)
    return _classes[name]


def lanes_of(f, xs):
    return (np.asarray(xs) - f.own[2]) % 64


# ---------------------------------------------------------------- independence
def test_restatement_and_fixtures_import_nothing_of_the_project():
    for mod in (cr, fx):
        src = open(mod.__file__).read()
        imports = [ln.strip() for ln in src.splitlines() if ln.startswith(("import ", "from "))]
        assert imports == ["import numpy as np"], imports


# ---------------------------------------------------------------- restatement == oracle
@pytest.mark.parametrize("name", list(UNIQ))
def test_uniqueness_restatement_equals_the_oracle(name):
    f = UNIQ[name]
    got = classes(name)[0]
    want = orc.uniqueness_pass(f.p, f.q, f.own, f.oth)
    assert got.dtype == want.dtype == f.p.dtype
    assert np.array_equal(got, want), diff_report(name, got, want)
    if f.chain:
        for a, b, ma, mb in ((f.p, f.q, f.own, f.oth), (f.q, f.p, f.oth, f.own)):
            g0, g1 = cr.uniqueness(a, b, ma, mb)
            w0, w1 = orc.uniqueness(a, b, ma, mb)
            assert np.array_equal(g0, w0) and np.array_equal(g1, w1), name


def parity_random_case(seed):
    """The inputs of test_gpu_parity.test_random_inputs_constraint_stages, built as that test builds them."""
    from test_gpu_parity import _rand_maps
    rng = np.random.default_rng(100 + seed)
    H, W = 72, 200 + 7 * seed
    d0, m0 = _rand_maps(seed, H, W, p_nomatch=0.15 * seed)
    d1, m1 = _rand_maps(50 + seed, H, W, p_nomatch=0.2)
    r = 2
    XL = int(rng.integers(r, 12)); XR = W - 1 - int(rng.integers(r, 12))
    own = (r + seed, H - 1 - r - seed, XL, XR, XR - XL + 1, H - 2 * (r + seed))
    oth = (r, H - 1 - r, XL + 3, XR - 5, XR - XL - 7, H - 2 * r)
    p = d0.copy(); q = d1.copy()
    ys, xs = np.nonzero(p != NOMATCH)
    for y, x in list(zip(ys, xs))[::3]:
        t = x + int(p[y, x])
        if 0 <= t < W:
            q[y, t] = -p[y, x] + int(rng.integers(-2, 3))
    pf = np.where(p == NOMATCH, float(NOMATCH), p + rng.normal(0, 0.4, p.shape))
    qf = np.where(q == NOMATCH, float(NOMATCH), q + rng.normal(0, 0.4, q.shape))
    return d0, m0, own, oth, p, q, pf, qf


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_restatements_equal_the_oracle_on_the_parity_tests_random_maps(seed):
    d0, m0, own, oth, p, q, pf, qf = parity_random_case(seed)
    for nm, a, b in (("smooth", cr.smooth_constraint(d0, own), orc.smooth_constraint(d0, own)),
                     ("order", cr.order_constraint(d0, own), orc.order_constraint(d0, own)),
                     ("median", cr.median_filter(d0, m0, own), orc.median_filter(d0, m0, own)),
                     ("uniq16", cr.uniqueness_pass(p, q, own, oth)[0], orc.uniqueness_pass(p, q, own, oth)),
                     ("uniq64", cr.uniqueness_pass(pf, qf, own, oth)[0], orc.uniqueness_pass(pf, qf, own, oth))):
        assert np.array_equal(a, b), diff_report("%s seed %d" % (nm, seed), a, b)


def test_smooth_and_median_restatements_equal_the_reference_goldens():
    G = np.load(os.path.join(GOLD, "ref_stages_golden.npz"))
    n = len([k for k in G.files if k.startswith("in__sm_disp_")])
    assert n == 7
    for i in range(n):
        d, mk, own = G["in__sm_disp_%d" % i], G["in__sm_mask_%d" % i], tuple(int(v) for v in G["in__sm_margin_%d" % i])
        got = cr.smooth_constraint(d, own)
        assert np.array_equal(got, G["ref__sm_smooth_%d" % i]), diff_report("smooth golden %d" % i, got, G["ref__sm_smooth_%d" % i])
        got = cr.median_filter(d, mk, own)
        assert np.array_equal(got, G["ref__sm_median_%d" % i]), diff_report("median golden %d" % i, got, G["ref__sm_median_%d" % i])


ORDER_DENSE_MAX = 700     # valid pixels per row up to which the dense matrix is used


def test_order_and_uniqueness_restatements_equal_the_reference_goldens():
    G = np.load(os.path.join(GOLD, "ref_probe_golden.npz"))
    n_oc = len([k for k in G.files if k.startswith("in__oc_disp_")])
    n_uq = len([k for k in G.files if k.startswith("in__uq_p_")])
    assert (n_oc, n_uq) == (7, 6)
    done = 0
    for i in range(n_oc):
        d, m = G["in__oc_disp_%d" % i], tuple(int(v) for v in G["in__oc_margin_%d" % i])
        if (d[m[0]:m[1] + 1, m[2]:m[3] + 1] != NOMATCH).sum(axis=1).max() > ORDER_DENSE_MAX:
            continue                                     # the C2-shaped rows of ~2000 pixels: beyond the dense restatement
        got = cr.order_constraint(d, m)
        assert np.array_equal(got, G["ref__oc_out_%d" % i]), diff_report("order golden %d" % i, got, G["ref__oc_out_%d" % i])
        done += 1
    assert done >= 4
    for i in range(n_uq):
        m = [int(v) for v in G["in__uq_margins_%d" % i]]
        d0, d1 = cr.uniqueness(G["in__uq_p_%d" % i], G["in__uq_q_%d" % i], tuple(m[:6]), tuple(m[6:]))
        assert np.array_equal(d0, G["ref__uq_out0_%d" % i]) and np.array_equal(d1, G["ref__uq_out1_%d" % i]), i


def test_arma_median_truncates_the_half_difference():
    assert cr.arma_median([-7, -4]) == -6 and cr.arma_median([-4, -7, -9, -1]) == -6      # (lo + hi) / 2 in C would give -5
    assert cr.arma_median([3, 8]) == 5 and cr.arma_median([5, 1, 9]) == 5


# ---------------------------------------------------------------- the uniqueness fixtures reach what they are for
@pytest.mark.parametrize("nm", ["s16", "f64"])
@pytest.mark.parametrize("sign", ["pos", "neg"])
def test_long_runs_cross_two_chunk_boundaries_and_die_with_their_head(nm, sign):
    f = UNIQ["long_%s_%s" % (sign, nm)]
    new, cls, run = classes("long_%s_%s" % (sign, nm))
    XL, XR = f.own[2], f.own[3]
    xs = np.arange(XL + 21, XL + 156)
    assert cls[0, XL + 20] == cr.DIRECT and (cls[0, xs] == cr.BY_PREV).all()
    assert run[0, xs[-1]] == 135 >= 130 and run[0, xs[0]] == 1
    assert lanes_of(f, xs[0]) == 21 and (xs[0] - XL) // 64 == 0 and (xs[-1] - XL) // 64 == 2      # chunks 0, 1 and 2
    # only the head differs between rows 0 and 1 ...
    assert np.array_equal(f.p[0], f.p[1]) and (f.q[0] != f.q[1]).sum() == 1
    # ... and the whole former run dies with it, although every pixel's own test on the input held
    assert cls[1, XL + 20] == cr.KILLED and (cls[1, xs] == cr.CHAIN_KILLED).all() and (new[1, XL:XR + 1] == NOMATCH).all()
    # from XL, on the untouched p[XL-1]
    xs = np.arange(XL, XL + 141)
    assert f.p[2, XL - 1] != NOMATCH and (cls[2, xs] == cr.BY_PREV).all() and run[2, xs[-1]] == 141
    assert cls[3, XL] == cr.KILLED and (cls[3, xs[1:]] == cr.CHAIN_KILLED).all()
    # kept by p[x+1]: at lane 63 twice (p[x+1] is lane 0 of the next chunk) and at XR (p[XR+1] is outside the margin)
    for x in (XL + 63, XL + 127, XR):
        assert cls[4, x] == cr.BY_NEXT and new[4, x] != NOMATCH
    assert list(lanes_of(f, [XL + 63, XL + 127])) == [63, 63]
    if sign == "neg":
        assert (f.p[0, XL + 20:XL + 156] < 0).all()


@pytest.mark.parametrize("name", ["lanes_pos_s16", "lanes_pos_f64", "lanes_neg_dead_s16", "lanes_neg_dead_f64"])
def test_runs_of_every_length_end_at_every_lane(name):
    f = UNIQ[name]
    new, cls, run = classes(name)
    XL = f.own[2]
    seen = set()
    for y in range(f.p.shape[0]):
        xs = np.nonzero(f.p[y] != NOMATCH)[0]
        head, body = xs[0], xs[1:]
        assert (np.diff(xs) == 1).all()
        if "dead" in name:
            assert cls[y, head] == cr.KILLED and (cls[y, body] == cr.CHAIN_KILLED).all()
        else:
            assert cls[y, head] == cr.DIRECT and (cls[y, body] == cr.BY_PREV).all() and run[y, body[-1]] == len(body)
        seen.add((len(body), int(lanes_of(f, body[-1]))))
    assert seen == {(L, lane) for L in fx.RUN_LENGTHS for lane in fx.END_LANES}


def test_margin_widths_and_row_counts():
    assert {w for w, r in fx.WIDTH_ROWS} == {1, 63, 64, 65, 128, 129} and {r for w, r in fx.WIDTH_ROWS} == {1, 3, 4, 5}
    for nm in ("s16", "f64"):
        for w, r in fx.WIDTH_ROWS:
            name = "width%d_rows%d_%s" % (w, r, nm)
            f = UNIQ[name]
            new, cls, run = classes(name)
            YL, YR, XL, XR = f.own[:4]
            assert (XR - XL + 1, YR - YL + 1) == (w, r)
            for y in range(r):
                if y % 3 == 0:       # the whole margin hangs on p[XL-1]: in a full chunk nothing but the carry decides
                    assert (cls[y, XL:XR + 1] == cr.BY_PREV).all() and run[y, XR] == w
                elif y % 3 == 1:
                    assert cls[y, XL] == cr.KILLED and (cls[y, XL + 1:XR + 1] == cr.CHAIN_KILLED).all()
                else:
                    assert cls[y, XR] == cr.BY_NEXT


@pytest.mark.parametrize("nm", ["s16", "f64"])
def test_clamped_and_empty_candidate_intervals(nm):
    n = dict(clamp_l=0, one=0, two=0, beyond_xr1=0, next_row=0, next_row_kept=0, beyond_buffer=0, half_pos=0, half_neg=0,
             minus_one_zero=0)
    sums = {s: 0 for s in (2 - fx.E40, 2.0, 2 + fx.E40)}
    for seed in (1, 2, 3):
        name = "clamps%d_%s" % (seed, nm)
        f = UNIQ[name]
        new, cls, run = classes(name)
        H, W = f.p.shape
        XL1, XR1 = f.oth[2], f.oth[3]
        assert f.own[1] == H - 1
        qf = f.q.ravel()
        for (y, x), (raw, bl, br) in fx.uniq_intervals(f.p, f.own, f.oth).items():
            v = f.p[y, x].item()
            n["clamp_l"] += raw < XL1
            n["one"] += bl == XR1 == br
            n["two"] += bl == XR1 - 1 and br == XR1
            if bl > XR1:
                assert cls[y, x] != cr.DIRECT
                n["beyond_xr1"] += bl + 1 < W
                n["next_row"] += bl + 1 >= W and y < H - 1
                n["next_row_kept"] += bl + 1 >= W and y < H - 1 and cls[y, x] in (cr.BY_NEXT, cr.BY_PREV)
                n["beyond_buffer"] += bl + 1 >= W and y == H - 1
                if bl + 1 >= W and y == H - 1:
                    assert cls[y, x] in (cr.KILLED, cr.CHAIN_KILLED)       # NOMATCH is read there
            frac = v - np.trunc(v)
            n["half_pos"] += frac == 0.5
            n["half_neg"] += frac == -0.5
            n["minus_one_zero"] += -1 < v < 0
            i = y * W + bl + 1
            qv = qf[i] if i < H * W else NOMATCH
            for s in [qf[y * W + c] + v for c in range(bl, br + 1)] + [qv + f.p[y, x - 1], qv + f.p[y, x + 1]]:
                if abs(s) in sums:
                    sums[abs(s)] += 1
    for k in ("clamp_l", "one", "two", "beyond_xr1", "next_row", "next_row_kept", "beyond_buffer"):
        assert n[k] >= 3, n
    if nm == "f64":
        assert n["half_pos"] >= 10 and n["half_neg"] >= 10 and n["minus_one_zero"] >= 10, n
        assert min(sums.values()) >= 3, sums


@pytest.mark.parametrize("nm", ["s16", "f64"])
def test_plus_nomatch_groups_live_on_a_dead_neighbour(nm):
    """|q[boundary_L+1] + p[x-1]| < 2 with p[x-1] reading NOMATCH: kept when p[x-1] is invalid or was killed, killed when it is
    alive; the pixel chained on x follows x."""
    f = UNIQ["plus_nomatch_" + nm]
    new, cls, run = classes("plus_nomatch_" + nm)
    XL = f.own[2]
    kept = killed = 0
    for y in range(4):
        for x in np.nonzero((f.q[y] > 9000))[0]:
            near = abs(f.q[y, x].item() - 10000) < 2
            assert f.p[y, x] == 0 and f.p[y, x + 1] == 2
            if y == 0:
                assert f.p[y, x - 1] == NOMATCH
            elif y == 2:
                assert cls[y, x - 1] == cr.DIRECT
            else:
                assert cls[y, x - 1] == cr.KILLED
            lives = near and y != 2
            assert cls[y, x] == (cr.BY_PREV if lives else cr.KILLED), (y, x)
            assert cls[y, x + 1] == (cr.BY_PREV if lives else cr.CHAIN_KILLED), (y, x)
            kept += lives; killed += not lives
    assert kept >= 10 and killed >= 8
    assert sorted(int(v) for v in lanes_of(f, np.nonzero(f.q[3] > 9000)[0])) == [0, 0, 0, 63]


def test_threshold_triples_decide_at_two_exactly():
    f = UNIQ["thresholds_f64"]
    new, cls, run = classes("thresholds_f64")
    want = {0: cr.DIRECT, 1: cr.BY_NEXT, 2: cr.BY_PREV}
    x = 8
    for s in (2 - fx.E40, 2.0, 2 + fx.E40):
        for sign in (1.0, -1.0):
            for role in range(3):
                assert cls[role, x - 1] == cr.DIRECT
                assert cls[role, x] == (want[role] if s < 2 else cr.KILLED), (role, s, sign)
            x += 10


# ---------------------------------------------------------------- the order fixtures
def test_order_narrow_rows_are_what_they_are_built_to_be():
    f = fx.order_narrow()
    stats = []
    got = cr.order_constraint(f.d, f.own, stats)
    want = orc.order_constraint(f.d, f.own)
    assert np.array_equal(got, want), diff_report("order narrow", got, want)
    assert len(stats) == len(f.rows)
    ones = []
    for st, row in zip(stats, f.rows):
        assert st["n"] == row["n"]
        for key in ("components", "longest", "spread"):
            if key in row:
                assert st[key] == row[key], (row, {k: st[k] for k in ("n", "components", "longest", "spread", "removed")})
        if row["kind"] == "one":
            ones.append(st["n"])
            assert st["ends"] == [st["n"] - 1] and st["removed"] >= 2
        if row["kind"] == "spread":
            assert st["removed"] == 0
        if row["kind"] == "wide_spread":
            assert st["spread"] > st["n"] and st["removed"] >= 2
        if row["kind"] == "ends":
            assert set(row["ends"]) <= set(st["ends"]) and not set(range(63)) & set(st["ends"]) and not set(range(65, 127)) & set(st["ends"])
    assert sorted(set(ones)) == sorted(fx.ORDER_ONE_COMPONENT)       # 48 = ORD_BIG lies inside


def test_order_wide_rows_make_up():
    """What the wide rows consist of, from the narrow analogue of every kind (the dense restatement is too large at 10432
    columns): the same constructions at 480 columns."""
    f = fx.order_wide(480, inversions=12)
    stats = []
    got = cr.order_constraint(f.d, f.own, stats)
    assert np.array_equal(got, orc.order_constraint(f.d, f.own))
    by = dict(zip(fx.ORDER_WIDE_KINDS[:5], stats[:5]))
    assert by["ordered"]["n"] == 480 and by["ordered"]["components"] == 0 and by["ordered"]["removed"] == 0
    assert by["tied_by_both_ends"]["longest"] == 480 and by["tied_by_both_ends"]["removed"] == 2
    assert by["local_inversions"]["components"] >= 8 and by["local_inversions"]["longest"] <= 12
    assert by["every_second_random"]["n"] == 240 and by["every_second_random"]["removed"] >= 40
    assert by["one_pixel"]["n"] == 1
    for w in fx.ORDER_WIDE_WIDTHS:
        g = fx.order_wide(w)
        assert g.d.shape == (6, w + 2) and g.own[3] - g.own[2] + 1 == w
        x = np.arange(w + 2)
        m = np.where(g.d != NOMATCH, g.d.astype(np.int64) + x, 0)
        assert m.max() <= 32767 and m.min() >= -32768
    lds = lambda maxL: maxL * 6 + (maxL // 64 + 1) * 12 + (maxL // 48 + 1) * 4      # launch_order's request
    up = lambda w: (w + 63) & ~63
    assert lds(up(10432)) <= 65536 < lds(up(10433))


# ---------------------------------------------------------------- smooth / median at the 256-column blocks
@pytest.mark.parametrize("width", fx.BLOCK_WIDTHS)
def test_block_edge_cases_restated_equal_the_oracle(width):
    rel = set()
    for c in fx.block_cases(width):
        YL, YR, XL, XR = c.own[:4]
        H, W = c.d.shape
        assert XR - XL + 1 == width and XL == YL == c.inset and H - 1 - YR == c.inset
        rel.add((c.inset, max(-2, min(2, 2 * XR - W)), W - 1 - XR == c.inset))
        a, b = cr.smooth_constraint(c.d, c.own), orc.smooth_constraint(c.d, c.own)
        assert np.array_equal(a, b), diff_report("smooth %s" % (c.own,), a, b)
        a, b = cr.median_filter(c.d, c.mask, c.own), orc.median_filter(c.d, c.mask, c.own)
        assert np.array_equal(a, b), diff_report("median %s" % (c.own,), a, b)
    for inset in fx.BLOCK_INSETS:      # 2 XR below W, at W - 1, W, W + 1, above W; and the margin `inset` from every border
        assert {r[1] for r in rel if r[0] == inset} == {-2, -1, 0, 1, 2}
        assert (inset, 2, True) in rel


def test_median_map_has_every_window_count():
    f = fx.median_counts_map()
    k = np.full(f.d.shape, -1)
    got = cr.median_filter(f.d, f.mask, f.own, counts=k)
    assert np.array_equal(got, orc.median_filter(f.d, f.mask, f.own))
    YL, YR, XL, XR = f.own[:4]
    inside = np.zeros(f.d.shape, bool); inside[YL:YR + 1, XL:XR + 1] = True
    at_nomatch = np.bincount(k[inside & (f.d == NOMATCH)], minlength=7)
    at_valid = np.bincount(k[inside & (f.d != NOMATCH)], minlength=7)
    assert at_nomatch[:6].min() >= 1 and at_nomatch[6] == 0, at_nomatch      # the centre is one of the six
    assert at_valid[1:].min() >= 1 and at_valid[0] == 0, at_valid
    odd = {4: 0, 6: 0}
    for y, x in zip(*np.nonzero(inside & ((k == 4) | (k == 6)))):
        u = np.sort(f.d[y - 1:y + 2, x - 1:x + 1].ravel().astype(int))
        u = u[u != NOMATCH]
        lo, hi = u[len(u) // 2 - 1], u[len(u) // 2]
        odd[len(u)] += hi < 0 and (hi - lo) % 2 == 1
    assert odd[4] >= 5 and odd[6] >= 1, odd
