"""tests/pair_ends_restatement.py against the oracle and against answers written by hand (no GPU).

The GPU tests of tests/test_gpu_pair_ends.py hold k_pyramid.hip and k_cloud.hip to scipy's pyrDown and erosion, to summed-area
tables and to a numpy DisparityToCloud; here those references are held to oracle/stereo_oracle.c -- which shares no code with
them -- on the same inputs, and to values anyone can check with a pencil."""
import numpy as np
import pytest

from oracle import oracle as orc

import pair_ends_restatement as pe


# ---------------------------------------------------------------- pyrDown
@pytest.mark.parametrize("H,W", pe.PYR_SIZES, ids=lambda v: str(v))
def test_pyr_down_ref_equals_the_oracle(H, W):
    for C in (1, 3):
        for kind in pe.PYR_KINDS:
            a = pe.pyr_image(H, W, C, kind)
            want = orc.pyr_down(a)
            got = pe.pyr_down_ref(a)
            assert got.shape == want.shape == (((H + 1) // 2, (W + 1) // 2) + ((3,) if C == 3 else ()))
            assert np.array_equal(got, want), (H, W, C, kind)


def test_pyr_down_impulse_reproduces_the_weights():
    """The weights sum to 256 and the result is (sum + 128) >> 8, so an impulse of height 255 at (2i + dy, 2j + dx) gives
    (255 w(dy) w(dx) + 128) >> 8 at (i, j): the weight products 1 4 6 16 24 36 are all told apart."""
    w = {-2: 1, -1: 4, 0: 6, 1: 4, 2: 1}
    for ref in (pe.pyr_down_ref, orc.pyr_down):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                a = np.zeros((21, 23), np.uint8)
                a[10 + dy, 12 + dx] = 255
                out = ref(a)
                assert out[5, 6] == (255 * w[dy] * w[dx] + 128) >> 8
        # and the whole footprint of one impulse on an even site: rows / columns 2i-2 .. 2i+2 reach destinations i-1, i, i+1
        a = np.zeros((21, 23), np.uint8)
        a[10, 12] = 255
        out = ref(a).astype(int)
        want = np.zeros_like(out)
        for (i, wy) in ((4, 1), (5, 6), (6, 1)):
            for (j, wx) in ((5, 1), (6, 6), (7, 1)):
                want[i, j] = (255 * wy * wx + 128) >> 8
        assert np.array_equal(out, want)


def test_pyr_down_rounds_half_up():
    """Accumulator exactly k 256 + 128: the centre weight is 36, so a lone 32 gives 1152 = 4 x 256 + 128 -> 5, a lone 96
    gives 3456 = 13 x 256 + 128 -> 14; one less in the accumulator would give 4 and 13."""
    for ref in (pe.pyr_down_ref, orc.pyr_down):
        for val, want in ((32, 5), (96, 14), (160, 23), (224, 32)):
            a = np.zeros((9, 9), np.uint8)
            a[4, 4] = val
            assert (36 * val) % 256 == 128
            assert ref(a)[2, 2] == want == (36 * val + 128) >> 8


def test_pyr_down_white_and_the_smallest_sizes():
    for ref in (pe.pyr_down_ref, orc.pyr_down):
        for (H, W) in pe.PYR_SIZES:
            out = ref(np.full((H, W), 255, np.uint8))
            assert out.shape == ((H + 1) // 2, (W + 1) // 2) and (out == 255).all()
        assert ref(np.array([[77]], np.uint8)).tolist() == [[77]]                       # 1x1: every tap is the pixel
        # 1x2 [a b]: columns -2..2 reflect to a b a b a -> (1 + 6 + 1) a + (4 + 4) b, times the 16 of the rows
        assert ref(np.array([[10, 200]], np.uint8)).tolist() == [[(16 * (8 * 10 + 8 * 200) + 128) >> 8]]
        assert ref(np.array([[10], [200]], np.uint8)).tolist() == [[(16 * (8 * 10 + 8 * 200) + 128) >> 8]]
        assert ref(np.array([[255, 0]], np.uint8)).tolist() == [[128]]                  # 32640 + 128 = 128 x 256


# ---------------------------------------------------------------- erosion
def test_ellipse_footprint_by_hand():
    assert pe.ellipse_footprint(1).tolist() == [[True]]
    assert pe.ellipse_footprint(2).astype(int).tolist() == [[0, 1], [1, 1]]            # r = c = 1: dy = -1 -> dx 0; dy = 0 -> dx 1
    assert pe.ellipse_footprint(3).astype(int).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
    assert pe.ellipse_footprint(5).astype(int).tolist() == [[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]]


@pytest.mark.parametrize("k", pe.ERODE_KS)
def test_erode_ref_equals_the_oracle(k):
    for i, (H, W) in enumerate(pe.ERODE_SIZES):
        m = pe.erode_mask(H, W, 100 * k + i)
        want = orc.erode_ellipse(m, k)
        got = pe.erode_ref(m, k)
        assert np.array_equal(got, want), (k, H, W, int((got != want).sum()))


# ---------------------------------------------------------------- window sums
def test_box_sums_ref_against_a_triple_loop():
    img = np.random.default_rng(5).integers(0, 256, size=(9, 11, 3)).astype(np.uint8)
    v = img.astype(np.int64)
    for r in (1, 2, 4):
        S1, S2 = pe.box_sums_ref(img, r)
        assert S1.dtype == S2.dtype == np.int64 and S1.shape == S2.shape == (9, 11)
        for y in range(9):
            for x in range(11):
                s1 = s2 = 0
                if y - r >= 0 and y + r < 9 and x - r >= 0 and x + r < 11:
                    for j in range(-r, r + 1):
                        for i in range(-r, r + 1):
                            for c in range(3):
                                s1 += int(v[y + j, x + i, c])
                                s2 += int(v[y + j, x + i, c]) ** 2
                assert (S1[y, x], S2[y, x]) == (s1, s2), (r, y, x)
    S1, S2 = pe.box_sums_ref(img, 4)
    assert np.count_nonzero(S1) == 3 and np.count_nonzero(S2) == 3         # 9 x 11 at r = 4: one row of three windows
    S1, S2 = pe.box_sums_ref(img[:8], 4)
    assert not S1.any() and not S2.any()                                   # H < 2r + 1: nothing fits


def test_box_sums_ref_white_at_radius_15():
    S1, S2 = pe.box_sums_ref(np.full((33, 40, 3), 255, np.uint8), 15)
    assert 31 * 31 * 3 * 255 == 735165 and 31 * 31 * 3 * 255 * 255 == 187467075
    assert set(np.unique(S1[15:18, 15:25])) == {735165} and set(np.unique(S2[15:18, 15:25])) == {187467075}
    assert np.count_nonzero(S1) == 3 * 10


# ---------------------------------------------------------------- cloud
@pytest.mark.parametrize("case", pe.cloud_cases(), ids=pe.cloud_case_id)
def test_cloud_ref_equals_the_oracle(case):
    inp = pe.cloud_input(*case)
    xo, bo = orc.disparity_to_cloud(inp["d"], inp["mask"], inp["img"], inp["Q"], inp["scale"], inp["R"], inp["T"], inp["own"])
    xr, br = pe.cloud_ref(**inp)
    assert xr.shape == xo.shape and np.array_equal(br, bo)
    assert pe.same_values(xr, xo)
    geom, share, kind = case
    if kind == "none" or share == 0:
        assert len(xr) == 0
    else:
        assert len(xr) > 0
        if pe.CLOUD_GEOMS.index(geom) % 2 == 0:
            assert not np.isfinite(xr).all()          # the d == 0 pixel
    print(pe.cloud_case_id(case), len(xr), "points,", int((~np.isfinite(xr)).any(axis=1).sum()), "not finite")
