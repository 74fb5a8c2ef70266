"""The compiled reference's cv::Mat-allocating stages straight in front of the HIP stage entry points, through the C ABI (no
oracle in between): tests/golden/ref_stages_golden.npz holds inputs and what the reference's own SmoothConstraint
(.cpp:370-448), MedianFilter (.cpp:763-815), SetBoundary_smooth<short> (.cpp:817-942), Rematch (.cpp:499-570) and
LowestLevelInitialMatch (.cpp:170-227) returned for them (oracle/ref_probe on mat_storage.cpp's storage;
tests/test_oracle_stage_golden.py says what the inputs contain and asserts it).  k_smooth, k_median, k_setb_vert / k_setb_horiz,
the sparse rematch path and the lowest-level NCC argmax must come out bit for bit; the matchers also under the byte-wise NCC
kernel (option ncc_bytes = 1).

The module re-runs tests/test_oracle_stage_golden.py under the gpu mark, so the GPU box's own toolchain shows
oracle == reference next to HIP == reference.  Nothing here reads anything but the .npz."""
import numpy as np
import pytest

import test_oracle_stage_golden as cpu_side
from test_oracle_stage_golden import G, N_MT, N_SB, N_SM, margin, margins, masked_own, mt_case

pytestmark = pytest.mark.gpu
NOMATCH = -10000


@pytest.fixture(params=[0, 1], ids=["dot4", "ncc_bytes"])
def ncc_kernel(ctx, request):
    """The matcher cases run under both NCC kernels."""
    ctx.set_option("ncc_bytes", request.param)
    try:
        yield request.param
    finally:
        ctx.set_option("ncc_bytes", 0)


@pytest.mark.parametrize("i", range(N_SM))
def test_hip_smooth_constraint_equals_the_reference(ctx, i):
    d, own = G["in__sm_disp_%d" % i], margin("in__sm_margin_%d" % i)
    got, ref = ctx.smooth_constraint(d, own), G["ref__sm_smooth_%d" % i]
    assert np.array_equal(got, ref), "%d pixels differ" % (got != ref).sum()       # whole map: the input outside the margin


@pytest.mark.parametrize("i", range(N_SM))
def test_hip_median_filter_equals_the_reference(ctx, i):
    d, mk, own = G["in__sm_disp_%d" % i], G["in__sm_mask_%d" % i], margin("in__sm_margin_%d" % i)
    got, ref = ctx.median_filter(d, mk, own), G["ref__sm_median_%d" % i]
    assert np.array_equal(got, ref), "%d pixels differ" % (got != ref).sum()       # whole map: NOMATCH outside the margin


@pytest.mark.parametrize("i", range(N_SB))
def test_hip_set_boundary_smooth_equals_the_reference(ctx, i):
    d, mk = G["in__sb_disp_%d" % i], G["in__sb_mask_%d" % i]
    own, oth = margins("in__sb_margins_%d" % i)
    st, BL, BR = ctx.set_boundary_smooth(d, mk, own, oth)
    assert st == 0
    sel = masked_own(mk, own)       # defined (and consumed by Rematch) only on masked pixels of the own margin
    rl, rr = G["ref__sb_bl_%d" % i], G["ref__sb_br_%d" % i]
    assert np.array_equal(BL[sel], rl[sel]), "%d of %d BL differ" % ((BL != rl)[sel].sum(), sel.sum())
    assert np.array_equal(BR[sel], rr[sel]), "%d of %d BR differ" % ((BR != rr)[sel].sum(), sel.sum())


@pytest.mark.parametrize("i", range(N_MT))
def test_hip_lowest_level_match_equals_the_reference(ctx, ncc_kernel, i):
    A, B, mA, mB, r, own, oth = mt_case(i)
    got, ref = ctx.initial_match(A, B, mA, mB, r, 2, own, oth), G["ref__mt_lowest_%d" % i]
    assert np.array_equal(got, ref), "%d pixels differ" % (got != ref).sum()


@pytest.mark.parametrize("i", range(N_MT))
def test_hip_rematch_equals_the_reference(ctx, ncc_kernel, i):
    A, B, mA, mB, r, own, oth = mt_case(i)
    ds, ref = G["in__mt_disp_%d" % i], G["ref__mt_rematch_%d" % i]
    for k in range(len(ds)):
        st, got = ctx.rematch(A, B, mA, mB, r, own, oth, ds[k])
        assert st == 0
        assert np.array_equal(got, ref[k]), (k, int((got != ref[k]).sum()))


@pytest.mark.parametrize("i", range(N_MT))
def test_hip_set_boundary_on_the_rematch_maps_equals_the_reference(ctx, i):
    """The intervals the reference's Rematch scanned (its own SetBoundary_smooth call, :514), incl. the row where :938-939 sends
    the scan past the other margin."""
    A, B, mA, mB, r, own, oth = mt_case(i)
    sel = masked_own(mA, own)
    for k, d in enumerate(G["in__mt_disp_%d" % i]):
        st, BL, BR = ctx.set_boundary_smooth(d, mA, own, oth)
        assert st == 0
        assert np.array_equal(BL[sel], G["ref__mt_bl_%d" % i][k][sel]) and np.array_equal(BR[sel], G["ref__mt_br_%d" % i][k][sel]), k


# ---- oracle == reference and the fixture's coverage, shown on the GPU box as well ----------------------------------------
test_oracle_smooth_on_the_gpu_box = cpu_side.test_smooth_constraint
test_oracle_median_on_the_gpu_box = cpu_side.test_median_filter
test_oracle_set_boundary_on_the_gpu_box = cpu_side.test_set_boundary_smooth
test_oracle_lowest_level_match_on_the_gpu_box = cpu_side.test_lowest_level_initial_match
test_oracle_rematch_on_the_gpu_box = cpu_side.test_rematch
test_stage_fixture_cases_on_the_gpu_box = cpu_side.test_fixture_holds_the_stage_cases
test_stage_fixture_typo_on_the_gpu_box = cpu_side.test_set_boundary_golden_fires_the_bl_br_typo
test_stage_fixture_slip_on_the_gpu_box = cpu_side.test_smooth_golden_depends_on_the_south_east_slip
test_stage_fixture_median_counts_on_the_gpu_box = cpu_side.test_median_golden_has_every_window_count
test_stage_fixture_minus_one_rows_on_the_gpu_box = cpu_side.test_match_golden_has_rows_of_minus_one_scores
test_stage_fixture_rematch_widths_on_the_gpu_box = cpu_side.test_rematch_golden_has_intervals_of_every_width
