"""The kernels at the two ends of a pair at their own boundaries, through the C ABI, every comparison exact.

k_pyramid.hip (pyrDown, FindMargin, the NCC window-sum tables) and k_cloud.hip (erosion quick-accept, ordered compaction,
reprojection) otherwise see only what synth.py and the pipeline produce: even sizes, smooth and almost fully valid maps.  Here
they get odd and one-pixel sizes, widths around their 256 / 1024-column blocks, heights around their 16-row chunks, sparse
and empty clouds and truncated outputs, against references that share no code with them (tests/pair_ends_restatement.py:
scipy's correlate1d and grey_erosion, summed-area tables, numpy) and against the oracle."""
import numpy as np
import pytest

from oracle import oracle as orc

import pair_ends_restatement as pe
from helpers import diff_report

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- pyrDown
@pytest.mark.parametrize("H,W", pe.PYR_SIZES, ids=lambda v: str(v))
def test_pyr_down_odd_and_tiny_sizes(ctx, H, W):
    for C in (1, 3):
        for kind in pe.PYR_KINDS:
            a = pe.pyr_image(H, W, C, kind)
            got = ctx.pyr_down(a)
            want = pe.pyr_down_ref(a)
            assert got.shape == want.shape
            assert np.array_equal(got, want), diff_report("pyr_down %dx%d C%d %s against scipy" % (H, W, C, kind), got, want)
            assert np.array_equal(got, orc.pyr_down(a)), "pyr_down %dx%d C%d %s against the oracle" % (H, W, C, kind)


# ---------------------------------------------------------------- window sums
@pytest.mark.parametrize("r", pe.BOX_RADII)
def test_box_sums_every_radius_at_the_block_and_chunk_boundaries(ctx, r):
    for (H, W) in pe.box_sizes(r):
        for kind in ("random", "white"):
            img = pe.box_image(H, W, kind, seed=r)
            R1, R2 = pe.box_sums_ref(img, r)
            S1, S2 = ctx.box_sums(img, r)
            assert S1.dtype == S2.dtype == np.int32
            tag = "r %d %dx%d %s" % (r, H, W, kind)
            assert np.array_equal(S1, R1.astype(np.int32)), diff_report("S1 " + tag, S1, R1)
            assert np.array_equal(S2, R2.astype(np.int32)), diff_report("S2 " + tag, S2, R2)
            if H < 2 * r + 1 or W < 2 * r + 1:
                assert not S1.any() and not S2.any()


def test_box_sums_refuses_bad_arguments(ctx):
    from reconstruction_amd import RsmError
    img = pe.box_image(40, 40, "random")
    for r in (0, 16, -1):
        with pytest.raises(RsmError) as e:
            ctx.box_sums(img, r)
        assert e.value.code == -1
    import ctypes as C
    S = np.zeros((40, 40), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert ctx._lib.rsm_stage_box_sums(ctx._h, None, 40, 40, 2, p(S), p(S)) == -1
    assert ctx._lib.rsm_stage_box_sums(ctx._h, p(img), 40, 40, 2, None, p(S)) == -1
    assert ctx._lib.rsm_stage_box_sums(ctx._h, p(img), 40, 40, 2, p(S), None) == -1


# ---------------------------------------------------------------- FindMargin
FM_WIDTHS = [0, 1, 15, 16, 17, 33, 1025, 1041]   # W - 2r: the 16-byte path against the scalar tail, the 1024-column lane stride
FM_HEIGHTS = [0, 1, 15, 16, 17, 33]              # H - 2r: FM_ROWS = 16 rows per workgroup


def _fm_check(ctx, mask, r, tag):
    want = pe.find_margin(mask, r)
    assert orc.find_margin(mask, r).astuple() == want, tag + " (oracle against the restatement)"
    got = ctx.find_margin(mask, r).astuple()
    assert got == want, "%s: got %s expected %s" % (tag, got, want)
    return want


def _fm_masks(H, W, r):
    """(name, mask): inverted defaults, everything, single 255s at the scanned frame's corners, 255s just outside it."""
    yield "all254", np.full((H, W), 254, np.uint8)
    yield "all255", np.full((H, W), 255, np.uint8)
    if H - 2 * r > 0 and W - 2 * r > 0:
        for (y, x) in ((r, r), (r, W - 1 - r), (H - 1 - r, r), (H - 1 - r, W - 1 - r)):
            m = np.full((H, W), 254, np.uint8)
            m[y, x] = 255
            yield "corner(%d,%d)" % (y, x), m
    m = np.full((H, W), 254, np.uint8)       # the lines next to the frame on all four sides: not scanned
    m[:, r - 1] = 255
    m[:, W - r] = 255
    m[r - 1, :] = 255
    m[H - r, :] = 255
    yield "outside", m
    if H - 2 * r > 0 and W - 2 * r > 0:
        m = m.copy()
        m[r + (H - 2 * r) // 2, r + (W - 2 * r) // 3] = 255
        yield "outside+one", m


@pytest.mark.parametrize("r", [1, 5, 15])
def test_find_margin_at_the_kernels_boundaries(ctx, r):
    sizes = [(17 + 2 * r, wd + 2 * r) for wd in FM_WIDTHS] + [(hd + 2 * r, 33 + 2 * r) for hd in FM_HEIGHTS]
    for (H, W) in sizes:
        for name, m in _fm_masks(H, W, r):
            want = _fm_check(ctx, m, r, "r %d %dx%d %s" % (r, H, W, name))
            if name in ("all254", "outside") or H - 2 * r <= 0 or W - 2 * r <= 0:
                assert want[:4] == (H - 1 - r, r, W - 1 - r, r)      # the inverted defaults (.cpp:1014-1017)


def test_find_margin_lone_pixel_at_every_column(ctx):
    """W - 2r = 41 = two 16-byte loads and a 9-byte tail per row: the lone 255 visits every byte of both paths; 22 scanned
    rows, the pixel in the first row of the second workgroup."""
    r, H, W = 1, 24, 43
    y = r + 16
    for x in range(r, W - r):
        m = np.full((H, W), 254, np.uint8)
        m[y, x] = 255
        want = _fm_check(ctx, m, r, "lone 255 at (%d, %d)" % (y, x))
        assert want == (y, y, x, x, 1, 1)


# ---------------------------------------------------------------- cloud
def _cloud_equal(tag, xg, bg, xr, br):
    assert xg.shape == xr.shape, "%s: %d points, expected %d" % (tag, len(xg), len(xr))
    assert np.array_equal(bg, br), diff_report(tag + " bgr", bg, br)
    assert pe.same_values(xg, xr), diff_report(tag + " xyz", xg, xr)


@pytest.mark.parametrize("case", pe.cloud_cases(), ids=pe.cloud_case_id)
def test_cloud_on_constructed_maps(ctx, case):
    inp, (xr, br) = pe.cloud_reference(case)
    a = (inp["d"], inp["mask"], inp["img"], inp["Q"], inp["scale"], inp["R"], inp["T"], inp["own"])
    xg, bg = ctx.disparity_to_cloud(*a)
    xo, bo = orc.disparity_to_cloud(*a)
    print(pe.cloud_case_id(case), len(xr), "points")
    _cloud_equal("against the oracle", xg, bg, xo, bo)
    _cloud_equal("against the numpy restatement", xg, bg, xr, br)   # differs from the oracle's verdict only by contraction
    geom, share, kind = case
    assert (len(xr) == 0) == (share == 0 or kind == "none")


def test_cloud_truncated_by_max_points(ctx):
    case = (pe.CLOUD_GEOMS[3], 0.5, "patches")
    inp, (xr, br) = pe.cloud_reference(case)
    n = len(xr)
    assert n > 1000
    for cap in (0, 1, n - 1, n, n + 1):
        xyz, bgr, total = ctx.disparity_to_cloud(inp["d"], inp["mask"], inp["img"], inp["Q"], inp["scale"], inp["R"], inp["T"],
                                                 inp["own"], max_points=cap)
        assert total == n, "max_points %d: total %d, expected %d" % (cap, total, n)
        assert xyz.shape == (cap, 3) and bgr.shape == (cap, 3)
        m = min(n, cap)
        _cloud_equal("max_points %d" % cap, xyz[:m], bgr[:m], xr[:m], br[:m])
        assert not xyz[m:].any() and not bgr[m:].any(), "max_points %d: host arrays written beyond record %d" % (cap, m)


@pytest.mark.parametrize("gi", [0, 2], ids=["ksize6", "ksize34"])
def test_erosion_through_the_cloud_path_equals_scipy(ctx, gi):
    """rsm_stage_cloud has no eroded-mask output: with a map valid everywhere and a full-image margin the emitted pixels ARE
    the eroded mask's 255 set.  The image carries each pixel's index, so the colours name the pixels, in order."""
    geom = pe.CLOUD_GEOMS[gi]
    H, W = geom[:2]
    inp = pe.cloud_input(geom, 1.0, "patches")
    rng = np.random.default_rng(50 + gi)
    mask = inp["mask"].copy()
    for _ in range(12):                                   # lone holes as well: discs of the element's own shape
        mask[int(rng.integers(0, H)), int(rng.integers(0, W))] = int(rng.integers(0, 255))
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    img = np.stack([idx & 255, (idx >> 8) & 255, idx >> 16], axis=2).astype(np.uint8)
    d = np.full((H, W), 1.5)
    own = (0, H - 1, 0, W - 1, W, H)
    ksize = int(np.ceil(0.02 * H))
    assert ksize == (6, None, 34)[gi]
    want = np.flatnonzero(pe.erode_ref(mask, ksize) == 255)
    assert 0 < len(want) < H * W - 100
    xg, bg = ctx.disparity_to_cloud(d, mask, img, inp["Q"], inp["scale"], inp["R"], inp["T"], own)
    got = bg[:, 0].astype(np.int64) | (bg[:, 1].astype(np.int64) << 8) | (bg[:, 2].astype(np.int64) << 16)
    assert np.array_equal(got, want), "emitted %d pixels, eroded mask holds %d; first difference at %s" % (
        len(got), len(want), np.flatnonzero(got[:min(len(got), len(want))] != want[:min(len(got), len(want))])[:1])
    assert np.array_equal(orc.erode_ellipse(mask, ksize) == 255, pe.erode_ref(mask, ksize) == 255)
