"""The CPU oracle against the COMPILED reference's cv::Mat-allocating matching stages: SmoothConstraint (.cpp:370-448),
MedianFilter (.cpp:763-815), SetBoundary_smooth<short> (.cpp:817-942), Rematch (.cpp:499-570) and LowestLevelInitialMatch
(.cpp:170-227).  tests/golden/ref_stages_golden.npz holds seeded inputs and what the reference's own object code returned
for them (oracle/ref_probe, linked with mat_storage.cpp: cv::Mat storage stood in for by malloc / constant fill / free, nothing
that computes a pixel value; oracle/ref_probe/make_golden.py `stages` is the generating script).  Everything must agree bit for
bit, on whole maps.

These stages carry the reference's quirkiest lines -- the south-east byte-index slip (:423-424), the bl/br typo (:938-939),
the two-column median window (:792), the strict `>` scan from -1 -- so the second half of the module asserts, from the fixture
alone, that the inputs really reach them: a fixture that never fires the typo would pin nothing about it."""
import os

import numpy as np
import pytest

from oracle import oracle as orc

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_stages_golden.npz"))
NOMATCH = -10000


def _n(prefix):
    return len([k for k in G.files if k.startswith("in__" + prefix)])


N_SM, N_SB, N_MT = _n("sm_disp_"), _n("sb_disp_"), _n("mt_imgA_")
MT_KINDS = ("random", "two_level", "inverse", "flat_regions")     # case i: radius (1, 2, 5)[i // 4], texture MT_KINDS[i % 4]


def margin(key):
    return tuple(int(v) for v in G[key])


def margins(key):
    m = margin(key)
    return m[:6], m[6:]


def masked_own(mask, own):
    """The pixels on which BL / BR are defined (and consumed by Rematch): mask 255 inside the own margin."""
    YL, YR, XL, XR = own[:4]
    sel = np.zeros(mask.shape, bool)
    sel[YL:YR + 1, XL:XR + 1] = mask[YL:YR + 1, XL:XR + 1] == 255
    return sel


def mt_case(i):
    A, B, mA, mB = (G["in__mt_%s_%d" % (k, i)] for k in ("imgA", "imgB", "maskA", "maskB"))
    own, oth = margins("in__mt_margins_%d" % i)
    return A, B, mA, mB, int(G["in__mt_r_%d" % i][0]), own, oth


def test_fixture_holds_the_stage_cases():
    assert (N_SM, N_SB, N_MT) == (7, 18, 12)
    assert [int(G["in__mt_r_%d" % i][0]) for i in range(N_MT)] == [1] * 4 + [2] * 4 + [5] * 4
    shapes = sorted({(m[1] - m[0] + 1, m[3] - m[2] + 1) for m in (margin("in__sb_margins_%d" % i) for i in range(N_SB))})
    assert shapes == [(2, 70), (3, 64), (31, 63), (32, 128), (33, 129), (97, 321)]
    for i in range(N_SB):       # the other view's margin is narrower on both sides
        own, oth = margins("in__sb_margins_%d" % i)
        assert own[2] < oth[2] and oth[3] < own[3]


# ---- oracle == reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(N_SM))
def test_smooth_constraint(i):
    d, own = G["in__sm_disp_%d" % i], margin("in__sm_margin_%d" % i)
    got, ref = orc.smooth_constraint(d, own), G["ref__sm_smooth_%d" % i]
    assert np.array_equal(got, ref), "%d pixels differ" % (got != ref).sum()
    out = np.ones(d.shape, bool); out[own[0]:own[1] + 1, own[2]:own[3] + 1] = False
    assert np.array_equal(ref[out], d[out])            # outside the margin: the input
    assert (ref != d).sum() >= 10                      # the case really removes pixels


@pytest.mark.parametrize("i", range(N_SM))
def test_median_filter(i):
    d, mk, own = G["in__sm_disp_%d" % i], G["in__sm_mask_%d" % i], margin("in__sm_margin_%d" % i)
    got, ref = orc.median_filter(d, mk, own), G["ref__sm_median_%d" % i]
    assert np.array_equal(got, ref), "%d pixels differ" % (got != ref).sum()
    assert (ref[~masked_own(mk, own)] == NOMATCH).all()  # outside the margin and off the mask: NOMATCH


@pytest.mark.parametrize("i", range(N_SB))
def test_set_boundary_smooth(i):
    d, mk = G["in__sb_disp_%d" % i], G["in__sb_mask_%d" % i]
    own, oth = margins("in__sb_margins_%d" % i)
    st, BL, BR = orc.set_boundary_smooth(d, mk, own, oth)
    assert st == 0
    sel = masked_own(mk, own)
    assert np.array_equal(BL[sel], G["ref__sb_bl_%d" % i][sel]), int((BL != G["ref__sb_bl_%d" % i])[sel].sum())
    assert np.array_equal(BR[sel], G["ref__sb_br_%d" % i][sel]), int((BR != G["ref__sb_br_%d" % i])[sel].sum())
    # the oracle restates the stage store by store, so the intermediate values left on unmasked pixels agree as well
    assert np.array_equal(BL, G["ref__sb_bl_%d" % i]) and np.array_equal(BR, G["ref__sb_br_%d" % i])


@pytest.mark.parametrize("i", range(N_MT))
def test_lowest_level_initial_match(i):
    A, B, mA, mB, r, own, oth = mt_case(i)
    got, ref = orc.lowest_level_initial_match(A, B, mA, mB, r, own, oth), G["ref__mt_lowest_%d" % i]
    assert np.array_equal(got, ref), "%d pixels differ" % (got != ref).sum()
    assert (ref[own[1]] == NOMATCH).all()              # the row without a masked candidate inside the other margin
    assert (ref[~masked_own(mA, own)] == NOMATCH).all()


@pytest.mark.parametrize("i", range(N_MT))
def test_rematch(i):
    A, B, mA, mB, r, own, oth = mt_case(i)
    ds, ref = G["in__mt_disp_%d" % i], G["ref__mt_rematch_%d" % i]
    for k in range(len(ds)):
        st, got = orc.rematch(A, B, mA, mB, r, own, oth, ds[k])
        assert st == 0
        assert np.array_equal(got, ref[k]), (k, int((got != ref[k]).sum()))
        st, BL, BR = orc.set_boundary_smooth(ds[k], mA, own, oth)      # the intervals the reference's Rematch scanned
        assert np.array_equal(BL, G["ref__mt_bl_%d" % i][k]) and np.array_equal(BR, G["ref__mt_br_%d" % i][k])
        assert np.array_equal(ref[k][ds[k] != NOMATCH], ds[k][ds[k] != NOMATCH])   # matched pixels are left alone


# ---- what the fixture must contain, computed from the fixture alone -------------------------------------------------------
def test_set_boundary_golden_fires_the_bl_br_typo():
    """.cpp:938-939 (`if (br_src_[XL] > XR1) bl_src_[XL] = XR1`) assigns: a masked pixel at x = XL whose right bound stays
    above XR1 while its LEFT bound became XR1 -- with the 10000 start value and with a finite bound carried down a column."""
    fired = finite = 0
    for i in range(N_SB):
        own, oth = margins("in__sb_margins_%d" % i)
        YL, YR, XL, XR1 = own[0], own[1], own[2], oth[3]
        mk = G["in__sb_mask_%d" % i][YL:YR + 1, XL] == 255
        bl, br = G["ref__sb_bl_%d" % i][YL:YR + 1, XL], G["ref__sb_br_%d" % i][YL:YR + 1, XL]
        hit = mk & (br > XR1) & (bl == XR1)
        assert (bl[mk & (br > XR1)] == XR1).all()
        fired += int(hit.sum()); finite += int((hit & (br < 5000)).sum())
    assert fired >= 40 and finite >= 15, (fired, finite)
    for i in range(N_MT):   # ... and inside Rematch, where it makes the scan start at XR1 and run past the other margin
        own, oth = margins("in__mt_margins_%d" % i)
        y, XL, XR1 = own[0] + 2, own[2], oth[3]
        assert (G["ref__mt_bl_%d" % i][:, y, XL] == XR1).all() and (G["ref__mt_br_%d" % i][:, y, XL] == XR1 + 3).all()
        assert (G["ref__mt_rematch_%d" % i][:, y, XL] + XL >= XR1).all()


def smooth_restated(d, own, slip):
    """SmoothConstraint (.cpp:380-447) in plain Python; slip=False indexes :423-424 as 2x / 2x+2, what the line seems to mean."""
    YL, YR, XL, XR = own[:4]
    H, W = d.shape
    q = np.zeros((H, 2 * W), np.uint8)
    far = lambda a, b: abs(int(a) - int(b)) > 1
    for y in range(YL, YR + 1):
        for x in range(XL, XR + 1):
            if d[y, x] == NOMATCH:
                continue
            for yy, xx, tot_own, tot_oth in ((y, x + 1, 2 * x, 2 * x + 2), (y + 1, x - 1, 2 * x, 2 * x - 2), (y + 1, x, 2 * x, 2 * x),
                                             (y + 1, x + 1, x if slip else 2 * x, x + 2 if slip else 2 * x + 2)):
                if d[yy, xx] == NOMATCH:
                    continue
                q[y, tot_own] += 1
                q[yy, tot_oth] += 1
                if far(d[y, x], d[yy, xx]):
                    q[y, 2 * x + 1] += 1
                    q[yy, 2 * xx + 1] += 1
    out = d.copy()
    tot, eff = q[:, 0::2].astype(int), q[:, 1::2].astype(int)
    kill = (tot == 0) | (2 * eff > tot)
    kill[:YL], kill[YR + 1:], kill[:, :XL], kill[:, XR + 1:] = False, False, False, False
    out[kill] = NOMATCH
    return out, tot


def test_smooth_golden_depends_on_the_south_east_slip():
    """The byte-index slip of :423-424 decides pixels of the fixture: restated with the slip the stage equals the reference,
    restated with 2x / 2x+2 it does not -- where the slipped terms land inside the margin (XL < XR/2) and where they do not
    (XL > XR/2: the pixel's own south-east count is still missing).  `total == 0` occurs on valid pixels of the sparse map."""
    moved = {}
    for i in range(N_SM):
        d, own = G["in__sm_disp_%d" % i], margin("in__sm_margin_%d" % i)
        ref = G["ref__sm_smooth_%d" % i]
        with_slip, tot = smooth_restated(d, own, True)
        assert np.array_equal(with_slip, ref), i
        moved[i] = int((smooth_restated(d, own, False)[0] != ref).sum())
        if i == 1:
            inside = np.zeros(d.shape, bool); inside[own[0]:own[1] + 1, own[2]:own[3] + 1] = True
            assert ((tot == 0) & (d != NOMATCH) & inside).sum() >= 50
    assert margin("in__sm_margin_3")[2] > margin("in__sm_margin_3")[3] // 2 and margin("in__sm_margin_4")[2] < margin("in__sm_margin_4")[3] // 2
    assert moved[4] >= 30 and moved[0] >= 30 and moved[2] >= 30 and sum(moved.values()) >= 200, moved


def test_smooth_golden_has_differences_of_zero_one_and_two():
    """DifferOfDisparity is `abs > 1` (:3): east neighbours that differ by exactly 0, 1 and 2 are all plentiful."""
    for i in (0, 2, 4):
        d = G["in__sm_disp_%d" % i].astype(int)
        ok = (d[:, :-1] != NOMATCH) & (d[:, 1:] != NOMATCH)
        diff = np.abs(d[:, 1:] - d[:, :-1])[ok]
        assert min((diff == 0).sum(), (diff == 1).sum(), (diff == 2).sum()) >= 200


def median_counts(d, mk, own):
    """k of :792-795 for every masked pixel of the margin: valid samples in rows y-1..y+1, columns x-1 and x."""
    v = (d != NOMATCH).astype(int)
    k = np.zeros(d.shape, int)
    for dy in (-1, 0, 1):
        for dx in (-1, 0):
            k[1:-1, 1:] += v[1 + dy:d.shape[0] - 1 + dy, 1 + dx:d.shape[1] + dx]
    return k, masked_own(mk, own)


def test_median_golden_has_every_window_count():
    """Every valid count the two-column window can have, at NOMATCH centres (k = 0..5; >= 4 fills the pixel) and at valid ones
    (k = 1..6; <= 2 removes it), masks of 255 mixed with 0..254, and even counts whose two middle samples have an odd, negative
    sum -- where the integer mean of the two rounds toward one of them."""
    at_nomatch, at_valid = np.zeros(7, int), np.zeros(7, int)
    for i in range(N_SM):
        d, mk, own = G["in__sm_disp_%d" % i], G["in__sm_mask_%d" % i], margin("in__sm_margin_%d" % i)
        k, sel = median_counts(d, mk, own)
        at_nomatch += np.bincount(k[sel & (d == NOMATCH)], minlength=7)
        at_valid += np.bincount(k[sel & (d != NOMATCH)], minlength=7)
        ref = G["ref__sm_median_%d" % i]
        assert np.array_equal(ref[sel] != NOMATCH, np.where(d[sel] == NOMATCH, k[sel] >= 4, k[sel] > 2))
        if i < 6:
            assert (mk == 255).sum() > 1000 and (mk < 255).sum() > 300 and len(np.unique(mk)) > 100
    assert at_nomatch[:6].min() >= 50 and at_nomatch[6] == 0, at_nomatch
    assert at_valid[1:].min() >= 50 and at_valid[0] == 0, at_valid
    d, mk, own = G["in__sm_disp_5"], G["in__sm_mask_5"], margin("in__sm_margin_5")
    k, sel = median_counts(d, mk, own)
    odd_negative = mixed = 0
    for y, x in zip(*np.nonzero(sel & (k % 2 == 0) & (k >= 4))):
        u = np.sort(d[y - 1:y + 2, x - 1:x + 1].ravel().astype(int))
        u = u[u != NOMATCH]
        a, b = u[len(u) // 2 - 1], u[len(u) // 2]
        odd_negative += (a + b) % 2 == 1 and a + b < 0
        mixed += u[0] < 0 < u[-1]
    assert odd_negative >= 40 and mixed >= 100, (odd_negative, mixed)


def ncc_scores_numpy(A, B, y, x, cands, r):
    """fp64 NCC of the own window at (y, x) with the other view's windows at the candidate columns (numpy's summation order:
    good to ~1e-15, which is all the coverage assertions need)."""
    def vec(I, c):
        w = I[y - r:y + r + 1, c - r:c + r + 1].astype(np.float64).ravel()
        w = w - w.mean()
        n = np.linalg.norm(w)
        return w / (n if n else 1.0)
    vl = vec(A, x)
    return np.array([vl @ vec(B, c) for c in cands])


def test_match_golden_has_rows_of_minus_one_scores():
    """Two-level image against its exact inverse: in the checkerboard half of row YL + 1 the own pixels of the masked
    candidates' parity see scores of -1 to within rounding from EVERY candidate -- the scan's start value, where `>` against
    `>=` and the last bit of the reference's own summation decide between a match and NOMATCH.  Both outcomes occur."""
    pixels = unmatched = matched = 0
    for i in range(N_MT):
        if MT_KINDS[i % 4] != "inverse":
            continue
        A, B, mA, mB, r, own, oth = mt_case(i)
        y, W = own[0] + 1, A.shape[1]
        cands = [c for c in range(oth[2], oth[3] + 1) if mB[y, c] == 255]
        assert len(cands) >= 5
        ref = G["ref__mt_lowest_%d" % i]
        for x in range(max(own[2], W // 2 + r), own[3] + 1):
            if mA[y, x] != 255 or x % 2:
                continue
            s = ncc_scores_numpy(A, B, y, x, cands, r)
            assert np.abs(s + 1).max() < 1e-12
            pixels += 1
            unmatched += ref[y, x] == NOMATCH
            matched += ref[y, x] != NOMATCH
    assert pixels >= 30 and unmatched >= 3 and matched >= 3, (pixels, unmatched, matched)


def test_match_golden_has_exact_ties_and_flat_windows():
    """Two-level textures: the best score is shared by several candidates (first maximum wins); flat windows on either side
    (norm 0 -> 1) score 0 and still match."""
    tied = flat = 0
    for i in range(N_MT):
        A, B, mA, mB, r, own, oth = mt_case(i)
        ref = G["ref__mt_lowest_%d" % i]
        for y in range(own[0], own[1]):
            cands = [c for c in range(oth[2], oth[3] + 1) if mB[y, c] == 255]
            for x in range(own[2], own[3] + 1):
                if mA[y, x] != 255:
                    continue
                if MT_KINDS[i % 4] == "two_level":
                    s = ncc_scores_numpy(A, B, y, x, cands, r)
                    top = np.nonzero(s > s.max() - 1e-12)[0]
                    if len(top) > 1:
                        tied += 1
                        assert ref[y, x] + x in [cands[t] for t in top]
                if MT_KINDS[i % 4] == "flat_regions" and np.ptp(A[y - r:y + r + 1, x - r:x + r + 1]) == 0:
                    flat += ref[y, x] != NOMATCH
    assert tied >= 30 and flat >= 10, (tied, flat)


def test_rematch_golden_has_intervals_of_every_width():
    """Rematch scans [BL, BR] of every NOMATCH pixel under the mask: empty intervals (BL > BR: the pixel stays NOMATCH), widths
    1 to 12 and the whole other margin all occur; maps at about 2 %, 30 % and 90 % NOMATCH."""
    widths = np.zeros(200, int)
    empty = whole = 0
    for i in range(N_MT):
        A, B, mA, mB, r, own, oth = mt_case(i)
        ds, ref = G["in__mt_disp_%d" % i], G["ref__mt_rematch_%d" % i]
        bl, br = G["ref__mt_bl_%d" % i].astype(int), G["ref__mt_br_%d" % i].astype(int)
        frac = [(d[own[0]:own[1] + 1, own[2]:own[3] + 1] == NOMATCH).mean() for d in ds]
        assert frac[0] < 0.06 and 0.2 < frac[1] < 0.4 and frac[2] > 0.8, frac
        sel = masked_own(mA, own)[None] & (ds == NOMATCH)
        w = (br - bl + 1)[sel]
        empty += int((w <= 0).sum())
        assert (ref[sel & (br < bl)] == NOMATCH).all()
        widths += np.bincount(np.clip(w, 0, 199), minlength=200)
        whole += int((w == oth[3] - oth[2] + 1).sum())        # nothing known: the whole other margin
    assert empty >= 200 and whole >= 10, (empty, whole)
    assert widths[1:13].min() >= 10, widths[:13]
