"""The device part of Rectify (csrc/k_rectify.hip: k_rect_map, k_remap<1|3>, k_st_level, k_erode_gray) at its block edges,
wraps and table levels, against tests/rectify_restatement.py: the exact homography in long double, a padded whole-array
bilinear remap, scipy's grey erosion -- references that share no loop with the kernels.  (Equality with the oracle, whose loops
are the kernels', is asserted in tests/test_gpu_rectify.py; tests/test_rectify_restatement_cpu.py holds the oracle to the same
references on the same inputs, tests/rectify_edge_cases.py.)

  rect_map   one thread per row, 64 per block: 1 / 63 / 64 / 65 / 129 rows by 1 / 2 / 257 columns; the pair's R1 and R2, the
             identity, 0.3 rad about each axis, a pose with coordinates below -40 px (iu >> 5 and iu & 31 of negative iu), a
             principal point at 40 000 (the (short) cast wraps).  Every entry is rint(32 u); within 1e-6 of a tie either
             neighbour passes, for at most 1e-4 of a case's entries and 1e-5 of all
  remap      map widths 255 / 256 / 257 (256 threads per block), sources of 1x1, 1x9, 9x1, 37x53, one and three channels,
             int16 extremes, -1 and size - 1 planted, map2 over all 16 bits; byte for byte
  erosion    every ksize at which the sparse table gains a level and its neighbours, 96 / 192 (PyrmNum 6 / 7), 255 (the
             stage's limit); widths 255 / 256 / 257, 1 x W, H x 1, 7 x 5, a lone hole in the last column / row; byte for byte
  the chain  rectify_pair at PyrmNum 1, 3, 5 and 6; byte for byte"""
import time

import numpy as np
import pytest

import rectify_edge_cases as ec
from helpers import diff_report

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- rect_map
@pytest.mark.parametrize("case", ec.map_cases(), ids=ec.map_case_id)
def test_rect_map_is_the_rounded_homography(ctx, case):
    pose, W, H = case
    m1, m2 = ctx.rect_map(*ec.map_pose(pose), W, H)
    excused, dev = ec.check_map_case(case, m1, m2)
    print("rect_map %s: max |fixed - 32 u| %.9f, %d of %d entries excused" % (ec.map_case_id(case), dev, excused, W * H))


def test_rect_map_excused_share_over_all_cases(ctx):
    n, e = ec.check_map_total(ctx.rect_map)
    print("rect_map: %d cases, %d entries, %d within 1e-6 of a rounding tie" % (len(ec.map_cases()), n, e))


# ---------------------------------------------------------------- remap
@pytest.mark.parametrize("case", ec.remap_cases(), ids=ec.remap_case_id)
def test_remap_at_block_edges_and_int16_extremes(ctx, case):
    src, m1, m2, want = ec.remap_input(case)
    got = ctx.remap_linear(src, m1, m2)
    assert got.shape == want.shape
    assert np.array_equal(got, want), diff_report("remap " + ec.remap_case_id(case), got, want)


@pytest.mark.parametrize("C", [1, 3])
def test_remap_constant_source_under_all_fractions(ctx, C):
    src, m1, m2 = ec.all_fractions_input(C)
    out = ctx.remap_linear(src, m1, m2)
    assert (out == 255).all(), "the weights do not sum to 32768 under fraction index %s" % np.argwhere(out != 255)[:4].tolist()


def test_remap_lone_pixel_four_tap_values(ctx):
    src, m1, m2, want = ec.lone_pixel_input()
    got = ctx.remap_linear(src, m1, m2)
    assert np.array_equal(got, want), diff_report("lone pixel (rows: tap 00 01 10 11; columns: LONE_FRACTIONS)", got, want)
    got = ctx.remap_linear(src, m1, m2 | np.uint16(0xFC00))                    # map2 is read through & 1023
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- grey erosion
@pytest.mark.parametrize("k", ec.ERODE_KS)
def test_grey_erosion_at_table_levels_and_block_edges(ctx, k):
    t0 = time.perf_counter()
    refs = ec.erode_references(k)
    t1 = time.perf_counter()
    for (name, m), want in zip(ec.erode_images(k), refs):
        got = ctx.erode_ellipse_gray(m, k)
        assert np.array_equal(got, want), diff_report("ksize %d %s against scipy" % (k, name), got, want)
    print("erode ksize %d: %d images, reference %.2f s, kernels %.2f s" % (k, len(refs), t1 - t0, time.perf_counter() - t1))


# ---------------------------------------------------------------- the chain
@pytest.mark.parametrize("case", ec.CHAIN_CASES, ids=ec.chain_case_id)
def test_rectify_pair_equals_the_chain(ctx, case):
    N, lowest, radius = case
    raw, _, _ = ec.chain_input(case)
    t0 = time.perf_counter()
    want = ec.chain_reference(case)
    t1 = time.perf_counter()
    g = ctx.rectify_pair(raw["K"], raw["E"], raw["origin"], lowest, N, raw["image"], raw["mask"], radius=radius)
    assert g["size"] == (lowest[0] << (N - 1), lowest[1] << (N - 1))
    for v in range(2):
        assert np.array_equal(g["image"][v], want["image"][v]), diff_report("image %d" % v, g["image"][v], want["image"][v])
        assert np.array_equal(g["mask"][v], want["mask"][v]), diff_report("mask %d" % v, g["mask"][v], want["mask"][v])
    t2 = time.perf_counter()
    n, e = ec.check_chain_maps(case)                      # the maps the reference images were made over, both views
    print("chain %s: ksize %d, reference %.2f s, GPU %.2f s; %d map entries, %d within 1e-6 of a rounding tie"
          % (ec.chain_case_id(case), 3 << (N - 1), t1 - t0, t2 - t1, n, e))
