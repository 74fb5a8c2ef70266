"""tests/rectify_restatement.py against the oracle and against answers written by hand (no GPU).

tests/test_gpu_rectify_edges.py holds k_rect_map, k_remap, k_st_level and k_erode_gray to the restatement; here the oracle
(oracle/rectify_oracle.c, which shares its loops with the kernels and no line with the restatement) is held to it on exactly
those inputs (tests/rectify_edge_cases.py), so that a failure on the GPU names the kernel and not the reference -- and the
restatement to values anyone can check with a pencil."""
import numpy as np
import pytest

from oracle import oracle as orc

import rectify_edge_cases as ec
import rectify_restatement as rr
from helpers import diff_report


# ---------------------------------------------------------------- by hand: the ellipse
def test_ellipse_footprints_written_out():
    """r = c = k / 2, row i holds [c - dx, c + dx] cut to the element, dx = cvRound(c sqrt((r^2 - dy^2) / r^2)), dy = i - r."""
    want = {1: ["1"],
            2: ["01", "11"],                                   # dy = -1: dx 0; dy = 0: dx 1, cut at the right edge
            3: ["010", "111", "010"],                          # the cross
            4: ["0010", "1111", "1111", "1111"],               # r = 2: dy = -2: dx 0; |dy| = 1: cvRound(1.73) = 2
            5: ["00100", "11111", "11111", "11111", "00100"]}
    for k, rows in want.items():
        assert ["".join("1" if b else "0" for b in row) for row in rr.ellipse_footprint(k)] == rows, k


def test_erosion_of_a_lone_hole_is_the_reflected_element():
    """A lone 7 among 255s: the result is 7 exactly where the element, centred on the pixel, covers the hole -- the footprint
    reflected through its anchor (k / 2, k / 2); for the even sizes that is not the footprint itself."""
    for ref in (rr.erode_ref, orc.erode_ellipse):
        for k in (2, 4, 5):
            m = np.full((11, 11), 255, np.uint8)
            m[5, 5] = 7
            out = ref(m, k)
            fp = rr.ellipse_footprint(k)
            a = k // 2
            want = np.full((11, 11), 255, np.uint8)
            for i in range(k):
                for j in range(k):
                    if fp[i, j]:                                # output (y, x) reads (y + i - a, x + j - a)
                        want[5 - (i - a), 5 - (j - a)] = 7
            assert np.array_equal(out, want), k


# ---------------------------------------------------------------- by hand: remap
REMAPS = (rr.remap_ref, orc.remap_linear)


@pytest.mark.parametrize("C", [1, 3])
def test_remap_constant_source_under_all_fractions(C):
    """(32 - fy)(32 - fx) + (32 - fy) fx + fy (32 - fx) + fy fx = 1024: times 32 the weights sum to 32768 = 1 << 15."""
    src, m1, m2 = ec.all_fractions_input(C)
    assert sorted(m2.ravel().tolist()) == list(range(1024))
    for ref in REMAPS:
        out = ref(src, m1, m2)
        assert out.shape == m2.shape + ((C,) if C == 3 else ()) and (out == 255).all()


def test_remap_lone_pixel_four_tap_values():
    src, m1, m2, want = ec.lone_pixel_input()
    k = {f: i for i, f in enumerate(ec.LONE_FRACTIONS)}
    assert want[0, k[(0, 0)]] == 200 and not want[1:, k[(0, 0)]].any()        # no fraction: tap 00 alone
    assert want[:, k[(31, 31)]].tolist() == [0, 6, 6, 188]                    # 32, 992, 992, 30752 of 32768
    assert want[:, k[(16, 0)]].tolist() == [100, 100, 0, 0]
    assert want[:, k[(16, 16)]].tolist() == [50, 50, 50, 50]
    assert want[:, k[(1, 1)]].tolist() == [188, 6, 6, 0]
    for ref in REMAPS:
        assert np.array_equal(ref(src, m1, m2), want)


def test_remap_rounds_half_up():
    """A lone 1 under the weight 16384 is exactly one half: (16384 + 16384) >> 15 = 1.  A rounding constant of 16383 gives 0."""
    src = np.zeros((3, 3), np.uint8)
    src[1, 1] = 1
    m1 = np.array([[[1, 1]]], np.int16)
    m2 = np.array([[16]], np.uint16)                                          # fx = 16, fy = 0: w00 = 32 * 16 * 32 = 16384
    for ref in REMAPS:
        assert ref(src, m1, m2).tolist() == [[1]]


def test_remap_border_taps_are_zero_one_side_at_a_time():
    """An all-255 source of 4 x 6: at sx = -1 only the right taps are inside, at sx = Ws - 1 only the left ones, and the same
    in y; the result is 255 times the inside weights, (255 * 1024 f' + 16384) >> 15 with f' the inside share of 32."""
    Hs, Ws = 4, 6
    src = np.full((Hs, Ws), 255, np.uint8)
    for fx, fy in ((5, 9), (31, 1), (16, 16), (1, 30)):
        m2 = np.full((1, 1), fy * 32 + fx, np.uint16)
        for (sx, sy, inside) in ((-1, 1, fx), (Ws - 1, 1, 32 - fx), (2, -1, fy), (2, Hs - 1, 32 - fy),
                                 (-1, -1, None), (Ws - 1, Hs - 1, None), (-2, 1, 0), (Ws, 1, 0), (2, -2, 0), (2, Hs, 0)):
            m1 = np.array([[[sx, sy]]], np.int16)
            if inside is None:                                                # a corner: one tap of the four
                w = (fx if sx < 0 else 32 - fx) * (fy if sy < 0 else 32 - fy) * 32
            else:
                w = inside * 32 * 32
            for ref in REMAPS:
                assert ref(src, m1, m2).tolist() == [[(255 * w + 16384) >> 15]], (fx, fy, sx, sy)


def test_remap_reads_map2_through_its_ten_low_bits():
    src, m1, m2, want = ec.lone_pixel_input()
    for ref in REMAPS:
        assert np.array_equal(ref(src, m1, m2 | np.uint16(0xFC00)), want)


# ---------------------------------------------------------------- by hand: the maps
def test_exact_map_of_the_identity():
    """R = I and newA = A: (x, y, w) = A^-1 (j, i, 1) and u = fx x + u0 = j."""
    A = np.array([[704.0, 0, 323.0], [0, 711.04, 238.0], [0, 0, 1.0]])
    u32, v32 = rr.exact_map(A, np.eye(3), A, 9, 5)
    assert u32.dtype == v32.dtype == np.longdouble and u32.shape == (5, 9)
    j, i = np.meshgrid(np.arange(9), np.arange(5))
    assert float(np.abs(u32 - 32 * j).max()) < 1e-15 and float(np.abs(v32 - 32 * i).max()) < 1e-15
    m1, m2 = rr.fixed_maps(u32, v32)
    assert np.array_equal(m1[..., 0], j) and np.array_equal(m1[..., 1], i) and not m2.any()
    assert rr.map_agrees(m1, m2, u32, v32) == 0


def test_exact_map_of_a_shift_and_a_zoom():
    """newA = A with twice the focal length and the principal point moved: u = (j - u0') / 2 + u0, rows and columns apart."""
    A = np.array([[100.0, 0, 10.0], [0, 50.0, 20.0], [0, 0, 1.0]])
    newA = np.array([[200.0, 0, 4.0], [0, 100.0, 6.0], [0, 0, 1.0]])
    u32, v32 = rr.exact_map(A, np.eye(3), newA, 7, 3)
    j, i = np.meshgrid(np.arange(7), np.arange(3))
    assert float(np.abs(u32 - 32 * ((j - 4) / 2.0 + 10)).max()) < 1e-14
    assert float(np.abs(v32 - 32 * ((i - 6) / 2.0 + 20)).max()) < 1e-14


def test_exact_map_of_a_quarter_turn_roll():
    """R = a roll of 90 degrees, A = newA with square pixels: the source of (j, i) is u0 + (i - v0), v0 - (j - u0)."""
    A = np.array([[100.0, 0, 10.0], [0, 100.0, 20.0], [0, 0, 1.0]])
    R = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])                        # x' = R x: (x, y) = R^T (x', y') = (y', -x')
    u32, v32 = rr.exact_map(A, R, A, 6, 4)
    j, i = np.meshgrid(np.arange(6), np.arange(4))
    assert float(np.abs(u32 - 32 * (10 + (i - 20))).max()) < 1e-13
    assert float(np.abs(v32 - 32 * (20 - (j - 10))).max()) < 1e-13


def test_fixed_maps_split_negative_and_wrapping_values():
    """iu = -1 -> integer part -1, fraction 31 (arithmetic shift, not division); -33 -> -2, 31; 32 * 40000 + 7 -> the low 16
    bits of 40000 = -25536, fraction 7; iv fills bits 5..9."""
    u32 = np.array([[-1, -33, -32, 32 * 40000 + 7, 33]], np.longdouble)
    v32 = np.array([[0, 31, -1, 5, 32 * 32768]], np.longdouble)
    m1, m2 = rr.fixed_maps(u32, v32)
    assert m1[0, :, 0].tolist() == [-1, -2, -1, -25536, 1]
    assert m1[0, :, 1].tolist() == [0, 0, -1, 0, -32768]
    assert m2[0].tolist() == [31, 31 * 32 + 31, 31 * 32, 5 * 32 + 7, 1]
    assert rr.map_agrees(m1, m2, u32, v32) == 0


def test_map_agrees_excuses_ties_and_nothing_else():
    u32 = np.array([[10.5, 10.5, 10.5 + 5e-7, 10.5 + 2e-6, -3.5]], np.longdouble)
    v32 = np.zeros((1, 5), np.longdouble)

    def maps(iu):
        iu = np.array([iu], np.int64)
        return np.stack([iu >> 5, 0 * iu], axis=-1).astype(np.int16), (iu & 31).astype(np.uint16)
    assert rr.map_agrees(*maps([10, 11, 10, 11, -4]), u32, v32) == 4          # entries 0, 1, 2 and 4 lie within 1e-6 of a tie
    assert rr.map_agrees(*maps([11, 10, 11, 11, -3]), u32, v32) == 4
    for bad in ([12, 11, 11, 11, -4], [10, 10, 10, 10, -4], [10, 11, 11, 11, -5], [10, 11, 11, 11, -2]):
        with pytest.raises(AssertionError):
            rr.map_agrees(*maps(bad), u32, v32)
    m1, m2 = maps([10, 11, 10, 11, -4])
    with pytest.raises(AssertionError):                                       # a fraction in the wrong five bits
        rr.map_agrees(m1, (m2 << 5).astype(np.uint16), u32, v32)
    with pytest.raises(AssertionError):                                       # bits above the ten
        rr.map_agrees(m1, m2 | np.uint16(1024), u32, v32)


# ---------------------------------------------------------------- the oracle on the GPU tests' inputs
@pytest.mark.parametrize("case", ec.map_cases(), ids=ec.map_case_id)
def test_oracle_maps_are_the_rounded_homography(case):
    pose, W, H = case
    ec.check_map_case(case, *orc.init_rectify_map(*ec.map_pose(pose), W, H))


def test_oracle_maps_excused_share_over_all_cases():
    n, e = ec.check_map_total(orc.init_rectify_map)
    print("rect_map, oracle: %d cases, %d entries, %d within 1e-6 of a rounding tie" % (len(ec.map_cases()), n, e))


@pytest.mark.parametrize("case", ec.remap_cases(), ids=ec.remap_case_id)
def test_oracle_remap_equals_the_restatement(case):
    src, m1, m2, want = ec.remap_input(case)
    got = orc.remap_linear(src, m1, m2)
    assert np.array_equal(got, want), diff_report("remap " + ec.remap_case_id(case), got, want)


@pytest.mark.parametrize("k", ec.ERODE_KS)
def test_oracle_grey_erosion_equals_scipy(k):
    for (name, m), want in zip(ec.erode_images(k), ec.erode_references(k)):
        got = orc.erode_ellipse(m, k)
        assert np.array_equal(got, want), diff_report("ksize %d %s" % (k, name), got, want)


def test_erosion_inputs_reach_what_they_are_for():
    """The planted images: the hole in the last column / row comes back as the element's shape cut by the image; the large
    elements are wider and higher than every image they meet."""
    for k in ec.ERODE_KS:
        imgs, refs = dict(ec.erode_images(k)), dict(zip((n for n, _ in ec.erode_images(k)), ec.erode_references(k)))
        assert (refs["last_column_12x70"][5] == 17).sum() == min(k - k // 2, 70)   # the anchor row and column are full: k - k / 2 of their pixels see the hole
        assert (refs["last_row_40x17"][:, 8] == 23).sum() == min(k - k // 2, 40)
        assert set(np.unique(refs["last_column_12x70"])) <= {17, 255}
        assert imgs["7x5"].shape == (7, 5) and imgs["1x261"].shape == (1, 261) and imgs["261x1"].shape == (261, 1)


@pytest.mark.parametrize("case", ec.CHAIN_CASES, ids=ec.chain_case_id)
def test_oracle_rectify_pair_equals_the_chain(case):
    raw, _, _ = ec.chain_input(case)
    want = ec.chain_reference(case)
    o = orc.rectify_pair(raw["K"], raw["E"], raw["origin"], raw["lowest"], raw["pyr_levels"], raw["image"], raw["mask"])
    for v in range(2):
        assert np.array_equal(o["image"][v], want["image"][v]), diff_report("image %d" % v, o["image"][v], want["image"][v])
        assert np.array_equal(o["mask"][v], want["mask"][v]), diff_report("mask %d" % v, o["mask"][v], want["mask"][v])
        assert 0 < (want["mask"][v] == 255).sum() < want["mask"][v].size
    n, e = ec.check_chain_maps(case)
    print("chain %s: %d map entries, %d within 1e-6 of a rounding tie" % (ec.chain_case_id(case), n, e))
