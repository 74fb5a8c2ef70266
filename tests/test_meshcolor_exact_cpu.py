"""The exact reference of the depth raster (tests/meshcolor_exact.py) without a GPU: the numpy restatement's
depth_buffer is held to it on every case the GPU file runs, the reference itself to answers worked out by hand, and the fixtures to what
they are for (how many decisions sit exactly on an edge, how many boxes each border cuts, how many faces lie on each side of the tier
switch).  The visibility scenes, whose answers are known beforehand, are put to the restatement's color() here and to the kernels in
tests/test_gpu_meshcolor_edges.py."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import meshcolor_exact as mx
import meshcolor_restatement as mr


def bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- the restatement against the exact reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mx.CASES)
def test_restatement_depth_buffer_is_the_exact_raster(name):
    c = mx.case(name)
    mx.hold(name, mr.depth_buffer(c.v, c.f, c.P, c.W, c.H), "restatement")


def test_excused_share_over_all_cases():
    dec = sum(mx.case_reference(n).decisions for n in mx.CASES)
    exc = sum(mx.case_reference(n).excused for n in mx.CASES)
    print("all %d cases: %d decisions, %d excused" % (len(mx.CASES), dec, exc))
    assert dec > 200000 and exc <= mx.CAP_ALL * dec


@pytest.mark.parametrize("name", ["tier_switch", "image_257x3", "box"])
@pytest.mark.parametrize("big_box", [1, mx.TIER_BIG_BOX, 1 << 20])
def test_restatement_item_counts_are_the_exact_boxes(name, big_box):
    c, R = mx.case(name), mx.case_reference(name)
    buf, drawn, big = mr.depth_buffer(c.v, c.f, c.P, c.W, c.H, True, big_box)
    assert (drawn, big) == R.items(big_box) and R.mismatches(buf) == 0


# ---- the reference against answers by hand ------------------------------------------------------------------------------------------------
def test_round_f32_by_hand():
    assert mx.round_f32(1, 2) == (bits(0.5),) * 3 + (False,)
    assert mx.round_f32(3, 1)[2] == bits(3.0) and mx.round_f32(1, 3)[2] == bits(1.0 / 3.0) == 0x3EAAAAAB
    # 1 + 2^-24 is the midpoint of 1 and 1 + 2^-23: to even, down; 1 + 3 2^-24 goes up to 1 + 2^-22
    assert mx.round_f32((1 << 24) + 1, 1 << 24) == (0x3F800000, 0x3F800001, 0x3F800000, True)
    assert mx.round_f32((1 << 24) + 3, 1 << 24) == (0x3F800001, 0x3F800002, 0x3F800002, True)
    # 2^-46 relative above the midpoint is not near, 2^-64 is -- and a double would lose it and round to even (double rounding)
    n, d = ((1 << 24) + 1) * (1 << 30) + (1 << 8), 1 << 54
    assert mx.round_f32(n, d) == (0x3F800000, 0x3F800001, 0x3F800001, False)
    n, d = ((1 << 24) + 1) * (1 << 40) + 1, 1 << 64
    assert mx.round_f32(n, d) == (0x3F800000, 0x3F800001, 0x3F800001, True) and np.float32(n / d) == np.float32(1.0)
    # subnormals: 2^-127 is 0x00400000, 2^-149 the least, 2^-150 the midpoint of 0 and it, 3 2^-150 that of the first two
    assert mx.round_f32(1, 1 << 127)[2] == 0x00400000 and mx.round_f32(1, 1 << 149)[2] == 1
    assert mx.round_f32(1, 1 << 150) == (0, 1, 0, True) and mx.round_f32(3, 1 << 151) == (0, 1, 1, False) and mx.round_f32(3, 1 << 150) == (1, 2, 2, True)
    assert mx.round_f32(1, 1 << 126)[2] == 0x00800000 == bits(2.0 ** -126)
    # the carry into the next binade and the overflow
    assert mx.round_f32((1 << 25) - 1, 1 << 25)[1:3] == (0x3F800000, 0x3F800000)
    top = (1 << 128) - (1 << 104)
    assert mx.round_f32(top, 1)[2] == 0x7F7FFFFF and mx.round_f32(top + (1 << 103), 1)[2] == mx.F32_INF and mx.round_f32(1 << 130, 1)[2] == mx.F32_INF
    rng = np.random.default_rng(1)
    for x in np.concatenate([rng.uniform(0.0, 4.0, 200), 2.0 ** rng.uniform(-149, 127, 200)]):      # a double rounds once to float32
        fr = Fraction(float(x))
        assert mx.round_f32(fr.numerator, fr.denominator)[2] == bits(x)


def test_is_double_and_the_doubt_of_an_edge_function():
    assert mx.is_double(0) and mx.is_double((1 << 53) - 1) and mx.is_double(((1 << 53) - 1) << 70) and not mx.is_double((1 << 53) + 1)
    assert mx.edge_in_doubt(0, 0, 4, 4, 2, 2) == (0, False)                     # E = 0 in small integers: exact, no doubt
    assert mx.edge_in_doubt(0, 0, 4, 4, 2, 3) == (4, False)
    big = (1 << 60) + 1                                                       # 61 bits: the differences round in fp64
    assert mx.edge_in_doubt(0, 0, big, big, 5, 5) == (0, True)
    assert mx.edge_in_doubt(0, 0, big, big, 5, 6)[1] is False                  # |E| = 2^60 + 1 against a bound of about 2^12


def test_a_triangle_whose_three_edges_pass_through_centres():
    # (1, 1), (7, 3), (3, 7): x - 3 y + 2 <= 0, x + y <= 10, 3 x - y - 2 >= 0.  Area 16, 8 lattice points on the boundary ((4, 2); (6, 4),
    # (5, 5), (4, 6); (2, 4); the vertices), so by Pick 13 inside: 21 centres
    rows = {1: [1], 2: [2, 3, 4], 3: [2, 3, 4, 5, 6, 7], 4: [2, 3, 4, 5, 6], 5: [3, 4, 5], 6: [3, 4], 7: [3]}
    want = np.zeros((9, 10), bool)
    for y, xs in rows.items():
        want[y, xs] = True
    v = np.float32([[1, 1, 1], [7, 3, 1], [3, 7, 1]])
    for f in ([[0, 1, 2]], [[0, 2, 1]]):
        R = mx.reference(v, f, mx.EYE_P, 10, 9)
        assert np.array_equal(R.lo != 0, want) and np.array_equal(R.lo, R.hi) and set(R.lo[want].tolist()) == {bits(1.0)}
        assert (R.covered, R.on_edge, R.decisions, R.excused) == ([21], [8], 49, 0) and R.box == [(1, 7, 1, 7)]
    # depths 1, 2, 4 at the vertices: at (4, 2), the middle of the first edge, w = (1 + 1/2) / 2; at (3, 3), lambda = (16, 8, 8) / 32
    v = np.float32([[1, 1, 1], [14, 6, 2], [12, 28, 4]])
    R = mx.reference(v, [[0, 1, 2]], mx.EYE_P, 10, 9)
    assert R.lo[2, 4] == bits(0.75) and R.lo[1, 1] == bits(1.0) and R.lo[3, 7] == bits(0.5) and R.lo[7, 3] == bits(0.25)
    assert R.lo[3, 3] == bits((16 * 1.0 + 8 * 0.5 + 8 * 0.25) / 32.0) and np.array_equal(R.lo != 0, want)


def test_a_sliver_that_takes_exactly_one_centre():
    d = mx.D
    v = np.float32([[3 - 0.9375 * 7, 4 - 0.9375 * 3, 1], [3 + 0.9375 * 7 - 3 * d, 4 + 0.9375 * 3 + 7 * d, 1], [3 + 0.9375 * 7 + 3 * d, 4 + 0.9375 * 3 - 7 * d, 1]])
    R = mx.reference(v, [[0, 1, 2]], mx.EYE_P, 12, 9)
    assert R.covered == [1] and R.on_edge == [0] and R.lo[4, 3] == bits(1.0) and (R.lo != 0).sum() == 1
    R = mx.reference(v + np.float32([-3.0 / 256, 7.0 / 256, 0]), [[0, 1, 2]], mx.EYE_P, 12, 9)                 # pushed off its axis: none
    assert R.covered == [0] and not R.hi.any() and R.decisions > 0


def test_a_value_on_a_float32_midpoint_is_listed_as_excused():
    # (0, 0) at depth 1, (2^24, 0) at depth 2, (0, 2^24) at depth 1: w = 1 - x 2^-25, at x = 1 exactly the midpoint of 1 - 2^-24 and 1:
    # either neighbour passes, and the decision is counted (once in each of the two rows)
    v = np.float32([[0, 0, 1], [2.0 ** 25, 0, 2], [0, 2.0 ** 24, 1]])
    R = mx.reference(v, [[0, 1, 2]], mx.EYE_P, 3, 2)
    assert (R.lo[0, 1], R.hi[0, 1]) == (0x3F7FFFFF, 0x3F800000) == (R.lo[1, 1], R.hi[1, 1]) and R.excused_val == 2 and R.excused_cov == 0 and R.decisions == 6
    assert (R.lo[0, 0], R.hi[0, 0]) == (0x3F800000, 0x3F800000) == (R.lo[1, 0], R.hi[1, 0])
    assert (R.lo[0, 2], R.hi[0, 2]) == (0x3F7FFFFF, 0x3F7FFFFF)                # 1 - 2^-24, a float32
    got = mr.depth_buffer(v, [[0, 1, 2]], mx.EYE_P, 3, 2)
    assert R.mismatches(got) == 0 and got[0, 1] == 0x3F800000                 # fp64 holds w exactly and rounds it to even
    wrong = got.copy()
    wrong[0, 1] = 0x3F7FFFFE
    assert R.mismatches(wrong) == 1


def test_the_denormal_inverse_depth_by_hand():
    c, R = mx.case("denormal"), mx.case_reference("denormal")
    want = np.uint32([[0x00400000, 0x00400000], [0x00400000, 0]])
    assert np.array_equal(R.lo, want) and np.array_equal(R.hi, want) and R.on_edge == [3] and R.excused == 0
    assert np.array_equal(mr.depth_buffer(c.v, c.f, c.P, 2, 2), want)


def test_the_large_values_by_hand():
    c, R = mx.case("large"), mx.case_reference("large")
    assert (R.lo[6:] == bits(2.0)).all()                       # the FLT_MAX triangle at depth 1/2 in front of the 2^127 one at depth 1
    assert R.lo[2, 3] == bits(2.0 ** 120) and R.lo[1, 20] == bits(2.0 ** 120) and R.lo[1, 30] == bits(1.0) and R.lo[5, 40] == bits(2.0 ** 120)
    assert not R.lo[0].any() and R.box[5] is None and np.array_equal(R.lo, R.hi)
    with np.errstate(all="ignore"):
        assert not np.isfinite(mr.project(c.P, c.v[15:16])[0, 0] / np.float32(0.5))   # the skipped face's quotient overflows


# ---- the fixtures reach what they are for -------------------------------------------------------------------------------------------------
def test_expected_counts_by_construction():
    for name in ("slivers", "tiny_and_zero_area", "box", "denormal"):
        c, R = mx.case(name), mx.case_reference(name)
        assert len(c.expect) == len(c.f) and R.covered == list(c.expect), name
    sl = mx.case("slivers").expect
    # seven slivers of one centre and seven of none in turn, then the rows (columns 3 .. 44; the whole row three times; 10 .. 11), the
    # diagonals (31 centres; 36 of 51 inside the image; 6) and the columns (rows 2 .. 30; the whole column; 5 .. 6)
    assert sl == [1, 0] * 7 + [42, 48, 48, 48, 2] + [31, 36, 6] + [29, 36, 2]
    tz = mx.case("tiny_and_zero_area").expect
    assert tz.count(1) == 8 and tz.count(11) == 2 and tz.count(0) == 13


def test_cases_hold_edges_borders_and_both_tiers():
    on_edge = {n: sum(mx.case_reference(n).on_edge) for n in mx.CASES}
    print("decisions with an edge function exactly 0:", on_edge)
    assert on_edge["integer_soup"] >= 500 and on_edge["slivers"] >= 300 and on_edge["box"] >= 100 and on_edge["tier_switch"] >= 50
    assert on_edge["dyadic_soup_eye"] == on_edge["general_soup_eye"] == 0     # grids of 2^-12 and random vertices meet no centre
    R = mx.case_reference("box")
    clip = np.array(R.clip)[[b is not None for b in R.box]]
    left, right, top, bottom = clip.sum(axis=0)
    corners = [int((clip[:, a] & clip[:, b]).sum()) for a, b in ((0, 2), (1, 2), (0, 3), (1, 3))]
    print("box: cut left %d, right %d, top %d, bottom %d; at the corners %s; faces that draw nothing %d" % (left, right, top, bottom, corners, sum(b is None for b in R.box)))
    assert min(left, right, top, bottom) >= 6 and min(corners) >= 2
    c = mx.case("box")
    assert sum(b is None for b in R.box) >= 8                                # 2^-12 outside, or short of the first column / row
    u0 = mr.project(c.P, c.v[c.minus_zero_vertex:c.minus_zero_vertex + 1])[0]
    assert np.signbit(u0[0] / u0[2]) and u0[0] / u0[2] == 0 and R.box[-1] == (0, 3, 22, 24)
    # minima and maxima exactly on an integer and 2^-12 either side: the first nine pairs of faces
    assert [R.box[2 * k][0] for k in range(9)] == [10, 10, 10, 10, 10, 10, 11, 11, 11] and [R.box[2 * k + 1][1] for k in range(9)] == [30] * 3 + [29] * 3 + [30] * 3
    c, R = mx.case("tier_switch"), mx.case_reference("tier_switch")
    pixels = [(b[1] - b[0] + 1) * (b[3] - b[2] + 1) for b in R.box]
    assert [p > mx.TIER_BIG_BOX for p in pixels] == c.expect_big and pixels.count(12) == 6 and pixels.count(13) == 3
    assert R.items(mx.TIER_BIG_BOX) == (13, 5) and R.items(1) == (13, 12) and R.items(1 << 20) == (13, 0)
    for name, (W, H) in (("image_1x1", (1, 1)), ("image_1x40", (1, 40)), ("image_40x1", (40, 1)), ("image_257x3", (257, 3))):
        c, R = mx.case(name), mx.case_reference(name)
        assert (c.W, c.H) == (W, H) and R.lo.shape == (H, W) and (R.lo != 0).all() and len(set(R.lo.ravel().tolist())) > min(2, W * H - 1)


# ---- the visibility scenes against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mx.SCENES)
def test_restatement_answers_the_visibility_scenes(name):
    s = mx.scenes()[name]
    views = mr.views_of([[SimpleNamespace(P=P, image=img, mask=m) for P, img, m in pair] for pair in s.pairs])
    rgb0, rgb1, best, st = mr.color(s.v, s.f, views, "both", s.min_cos, s.depth_eps)
    mx.hold_scene(s, 0, rgb0, best)
    mx.hold_scene(s, 1, rgb1, best)


def test_the_scenes_are_what_they_claim():
    sc = mx.scenes()
    assert sorted(sc) == sorted(mx.SCENES)
    for s in sc.values():                                     # normals exactly (0, 0, -1); the centres exact
        N = mr.vertex_normals(s.v, s.f)
        assert not N[:, :2].any() and (N[s.probe, 2] < 0)
    s = sc["view_order_left_first"]
    assert np.array_equal(mr.cam_center(s.pairs[2][0][0]), [-3.0, 0.0, 0.0]) and np.array_equal(mr.cam_center(s.pairs[0][1][0]), [3.0, 0.0, 0.0])
    s = sc["undrawn_depth_4"]
    P = s.pairs[0][0][0]
    assert not mr.depth_buffer(s.v, s.f, P, 16, 12).any() and not mx.reference(s.v, s.f, P, 16, 12).hi.any()
    s = sc["depth_at_8.5"]
    R = mx.reference(s.v, s.f, s.pairs[0][0][0], 16, 12)
    assert (R.lo == bits(0.125)).all() and (R.hi == bits(0.125)).all()
    assert float(sc["depth_next_above_8.5"].v[4, 2]) == 8.5 + 2.0 ** -20
