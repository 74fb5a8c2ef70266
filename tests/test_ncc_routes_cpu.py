"""The restatement behind tests/test_gpu_ncc_routes.py, held to the kernel source and to the oracle (no GPU).

tests/ncc_routes.py restates which kernel of the NCC initial match takes which pixel (k_match.hip) and the candidate
interval every pixel scans.  Here: its constants are the source's, its intervals are the oracle's, and its case set reaches
both sides of every routing threshold -- checked before any GPU run."""
import time

import numpy as np

import ncc_routes as nr
from oracle import oracle as orc


def test_constants_are_the_kernel_source_s():
    got = nr.source_constants()
    assert got == dict(NCC_TX=nr.NCC_TX, NCC_WIDE=nr.NCC_WIDE, RG_SLOTS=nr.RG_SLOTS, RG_MIN=nr.RG_MIN,
                       RG_SLIDE_MIN=nr.RG_SLIDE_MIN, RG_MID_MIN=nr.RG_MID_MIN, RG_CC=nr.RG_CC, SL_COLS=nr.SL_COLS,
                       SL_DC=nr.SL_DC, RG_PX=nr.RG_PX, ncc_mid_default=(5, 64, 3, 96),
                       WIDE_WORKGROUPS=nr.WIDE_WORKGROUPS, slide_split=(12, 6)), got
    assert [nr.default_ncc_mid(r) for r in range(1, 8)] == [160, 160, 96, 96, 64, 64, 64]


def test_options_clamp_as_rsm_set_option():
    src = "".join(open(nr.K_MATCH.replace("k_match.hip", f)).read() for f in ("rsm_api.hip", "rsm_ctx.h"))   # rsm_set_option; struct rsm_ctx
    assert 'c->opt_ncc_mid = value <= 0 ? 0 : (int)std::max(8LL, std::min(value, 160LL));' in src
    assert '{"ncc_slide_max", &rsm_ctx::opt_ncc_slide_max, OPT_CLAMP, 0, 1000000},' in src   # a row of the option table, stored as ...
    assert 'o.kind == OPT_BOOL ? (int)(value != 0) : (int)std::max(o.lo, std::min(value, o.hi));' in src
    assert 'int opt_ncc_slide_max = 512;' in src
    assert nr.options(ncc_mid=1, ncc_slide_max=1 << 20) == dict(wide_rows=0, ncc_mid=8, ncc_slide_max=1000000)
    assert nr.options(ncc_mid=400) == dict(wide_rows=0, ncc_mid=160, ncc_slide_max=512)


def test_margins_are_the_oracle_s():
    for c in nr.cases():
        assert c.own == tuple(orc.find_margin(c.mask_own, c.r).astuple()), c.name
        assert c.oth == tuple(orc.find_margin(c.mask_oth, c.r).astuple()), c.name


def _oracle(c):
    if c.parent is None:
        return orc.lowest_level_initial_match(c.img_own, c.img_oth, c.mask_own, c.mask_oth, c.r, c.own, c.oth)
    return orc.high_level_initial_match(c.img_own, c.img_oth, c.mask_own, c.mask_oth, c.r, c.offset, c.own, c.oth, c.parent)


def test_restated_intervals_hold_the_oracle_s_columns():
    """On every case of the set: a column the oracle matched lies inside the restated interval, a pixel with an empty
    interval stays NOMATCH; on the 8-bit noise cases (view 1 = view 0 shifted by `shift` columns) the oracle finds the
    planted column whenever it lies inside the interval and view 1's mask holds it.  Also measures the oracle's cost."""
    t0 = time.time()
    planted = 0
    for c in nr.cases():
        d = _oracle(c)
        L, R, w = c.iv()
        ok = d != nr.NOMATCH
        ys, xs = np.nonzero(ok)
        col = xs + d[ok]
        assert (w[ok] > 0).all(), (c.name, "a match outside the scanned pixels")
        assert ((col >= L[ok]) & (col <= R[ok])).all(), (c.name, "a match outside the restated interval")
        if c.kind == "noise":
            ys, xs = np.nonzero(w > 0)
            pc = xs + c.shift
            inside = (pc >= L[ys, xs]) & (pc <= R[ys, xs])
            inside &= c.mask_oth[ys, np.clip(pc, 0, c.W - 1)] == 255
            assert (d[ys[inside], xs[inside]] == c.shift).all(), (c.name, "planted column missed")
            planted += int(inside.sum())
    dt = time.time() - t0
    print("oracle over the case set: %.1f s, %d planted columns found" % (dt, planted))
    assert planted > 10000


def test_mode1_intervals_carry_the_boundaries_as_the_oracle_does():
    """A hand-made parent row: anchors, a NOMATCH run with its boundary_R from the next anchor (i + trunc(2 s[i]) + offset
    + 1, i a PARENT column), a run with no anchor to its right (boundary_R carried), masked-out pixels (no update), and
    negative and fractional parent values (trunc toward zero)."""
    W, H, r, off = 60, 12, 1, 2
    parent = np.full((7, 32), float(nr.NOMATCH))
    p = 3                                                # own rows 5 and 6
    parent[p, 4] = 1.25                                  # x = 7, 8: c = x + trunc(3.0) = x + 3
    parent[p, 10] = -1.75                                # run cols 5..9 (x 9..18): R = 10 + trunc(-3.5) + 2 + 1 = 10
    parent[p, 12] = 7.0
    m0 = np.zeros((H, W), np.uint8)
    m0[5:7, 7:40] = 255
    m0[5:7, 12] = 0
    m1 = np.zeros((H, W), np.uint8)
    m1[2:10, 3:55] = 255
    own, oth = orc.find_margin(m0, r).astuple(), orc.find_margin(m1, r).astuple()
    L, R, w = nr.intervals(m0, own, oth, r, parent, off)
    assert (L[5, 7], R[5, 7]) == (8, 12) and (L[5, 8], R[5, 8]) == (9, 13)
    assert (L[5, 9], R[5, 9]) == (9, 10) and (L[5, 18], R[5, 18]) == (9, 10)      # boundary_L carried from x = 8
    assert w[5, 12] == 0                                                              # masked out
    assert (L[5, 19], R[5, 19]) == (max(19 + (-3) - 2, 3), 19 - 3 + 2)             # trunc(-3.5 + 0.5) = -3
    assert (L[5, 21], R[5, 21]) == (20 + (-3) - 2, 12 + 14 + 2 + 1)                # boundary_R from parent column 12
    assert (L[5, 24], R[5, 24]) == (24 + 14 - 2, 24 + 14 + 2)
    assert (L[5, 25], R[5, 25]) == (36, 40) and (L[5, 39], R[5, 39]) == (36, 40)    # no anchor right of col 12: both carried
    rng = np.random.default_rng(5)
    img0 = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    img1 = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    d = orc.high_level_initial_match(img0, img1, m0, m1, r, off, own, oth, parent)
    ok = d != nr.NOMATCH
    assert np.array_equal(ok, w > 0)                     # noise: every scanned pixel finds some column
    ys, xs = np.nonzero(ok)
    assert ((xs + d[ok] >= L[ok]) & (xs + d[ok] <= R[ok])).all()


def test_route_rule_on_small_rows():
    width = np.zeros((6, 1200), np.int64)
    width[0, :47] = 161                                  # 47 wide: k_ncc_wide
    width[1, :48] = 161                                  # 48: row GEMM
    width[2, :512] = 65                                  # 512 mid pixels at R = 5: a mid row, all of them wide, GEMM
    width[3, :511] = 65                                  # 511: not a mid row, 65 candidates stay in the band kernel
    width[4, :1024] = 512                                # 1024 wide, widest = ncc_slide_max: sliding sums
    width[5, :1024] = 513                                # widest 513: GEMM
    rt = nr.route(width, 5, {})
    assert rt["route"].tolist() == [1, 2, 2, 0, 3, 2]
    assert rt["wide"].tolist() == [47, 48, 512, 0, 1024, 1024]
    assert rt["worklist"] == 47 + 48 + 512 + 2048
    assert nr.route(width, 5, dict(wide_rows=1))["route"].tolist() == [1, 1, 0, 0, 1, 1]
    assert nr.route(width, 5, dict(wide_rows=3))["route"].tolist() == [1, 3, 3, 0, 3, 3]
    assert nr.route(width, 5, dict(ncc_slide_max=0))["route"].tolist() == [1, 2, 2, 0, 2, 2]
    assert nr.route(width, 2, {})["route"].tolist() == [1, 2, 0, 0, 3, 2]   # R = 2: no mid route by default


def test_case_set_reaches_every_side_of_every_threshold():
    """The restatement alone: before any GPU run the case set must reach both sides of every row of the threshold table."""
    got = set()
    for c in nr.cases():
        for o in c.opt_sets:
            got |= nr.sides(c, c.route(o))
    missing = nr.required_sides() - got
    assert not missing, sorted(missing, key=str)
