"""GPU parity: every HIP stage (through the C ABI) against the CPU oracle on the same seeded inputs.

Integer / index stages must be bit-exact.  fp64 stages: north_star's bar is 1e-3 relative; the tests hold the HIP path
to bit-exactness as well (REFINE_RTOL = 0): the refine data term is a bit-faithful fp64 restatement of WindowToVec +
arma::dot, sqrt and division are IEEE-exact on both sides, and the one libm call of the stage -- exp in the smoothness
weights -- is evaluated by the same fully specified routine in the oracle and on the GPU (oracle/stereo_oracle.c:
orc_exp_neg).  With the host's libm exp instead, one-ulp differences are amplified chaotically by the iteration
(test_libm_exp_sensitivity)."""
import numpy as np
import pytest

from oracle import oracle as orc
from reconstruction_amd import synth

from helpers import NOMATCH, cloud_scale, diff_report, host_libm_is_glibc_with_fma, libm_exp_stats, oracle_stages, refine_options

pytestmark = pytest.mark.gpu

CASES = {
    "s96x64_r2": dict(width=96, height=64, levels=2, radius=2, offset=2, pair=0),
    "s128x96_r2_neg_holes": dict(width=128, height=96, levels=3, radius=2, offset=2, pair=1, holes=True,
                                 mask_l0_width=20, border_l0=4),
    "s160x96_r5_off4": dict(width=160, height=96, levels=2, radius=5, offset=4, pair=2, border_l0=7),
    "s192x128_ellipse": dict(width=192, height=128, levels=3, radius=2, offset=2, pair=3, mask_kind="ellipse",
                             holes=True),
    "s640x256_r3_wide": dict(width=640, height=256, levels=2, radius=3, offset=2, pair=4, mask_l0_width=300,
                             border_l0=9),
    "s256x128_occluded": dict(width=256, height=128, levels=3, radius=2, offset=2, pair=5, occlude=True,
                              mask_l0_width=48, border_l0=5),
    "s320x160_occluded_neg_r4": dict(width=320, height=160, levels=2, radius=4, offset=3, pair=7, occlude=True,
                                     holes=True, mask_l0_width=120, border_l0=6),
    "s200x120_r7_single_level": dict(width=200, height=120, levels=1, radius=7, offset=2, pair=8, mask_l0_width=150,
                                     border_l0=12, d0_l0=5.0),
    "s512x384_5levels": dict(width=512, height=384, levels=5, radius=3, offset=2, pair=21, mask_l0_width=16,
                             holes=True, occlude=True),
    "s144x96_r1_r6": dict(width=144, height=96, levels=2, radius=1, offset=5, pair=9, occlude=True, mask_l0_width=50,
                          border_l0=4),
    "s288x160_r6": dict(width=288, height=160, levels=3, radius=6, offset=2, pair=10, mask_l0_width=40, border_l0=9),
    # radii 8..15: k_box_h_any, k_ncc_bytes by dispatch in all three modes, k_ncc_exact on windows of up to 2883 bytes
    "s192x128_r8": dict(width=192, height=128, levels=2, radius=8, offset=2, pair=3, holes=True, mask_l0_width=60, border_l0=2),
    "s224x144_r11_neg": dict(width=224, height=144, levels=2, radius=11, offset=3, pair=4, occlude=True, mask_l0_width=80,
                             border_l0=1),
    "s192x128_r15": dict(width=192, height=128, levels=2, radius=15, offset=2, pair=5, mask_l0_width=70, border_l0=1),
    "s384x256_r9_3levels": dict(width=384, height=256, levels=3, radius=9, offset=2, pair=6, holes=True, mask_l0_width=60,
                                border_l0=1),
}

_cache = {}


def stages(name):
    if name not in _cache:
        cfg = synth.config_small(**CASES[name])
        rec, fin = oracle_stages(cfg)
        _cache[name] = (cfg, rec, fin)
    return _cache[name]


REFINE_RTOL = 0.0


def fp_close(a, b, rel=REFINE_RTOL):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    na, nb = a == NOMATCH, b == NOMATCH
    assert np.array_equal(na, nb), "NOMATCH sets differ: %d vs %d" % (na.sum(), nb.sum())
    v = ~na
    if v.any():
        err = np.abs(a[v] - b[v]) / np.maximum(1.0, np.abs(b[v]))
        assert err.max() <= rel, "max rel err %.3e" % err.max()
        return float(err.max())
    return 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_pyramid_and_margins(ctx, name):
    cfg, rec, fin = stages(name)
    N = cfg.pyr_levels
    for k in range(N - 1, 0, -1):
        for v in range(2):
            g = ctx.pyr_down(fin["imgs"][k][v])
            assert np.array_equal(g, fin["imgs"][k - 1][v]), diff_report("pyr_down img L%d" % k, g, fin["imgs"][k - 1][v])
            g = ctx.pyr_down(fin["msks"][k][v])
            assert np.array_equal(g, fin["msks"][k - 1][v]), diff_report("pyr_down mask L%d" % k, g, fin["msks"][k - 1][v])
    for k in range(N):
        for v in range(2):
            assert ctx.find_margin(fin["msks"][k][v], cfg.radius).astuple() == orc.find_margin(fin["msks"][k][v], cfg.radius).astuple()


@pytest.mark.parametrize("name", list(CASES))
def test_integer_stages_bit_exact(ctx, name):
    cfg, rec, fin = stages(name)
    r, off = cfg.radius, cfg.offset
    imgs, msks = fin["imgs"], fin["msks"]
    fails = []
    for q in rec:
        k, st = q["level"], q["stage"]
        mg = q["mg"]
        tag = "%s L%d %s v%s" % (name, k, st, q.get("v"))
        if st == "initial":
            v = q["v"]; o = 1 - v
            g = ctx.initial_match(imgs[k][v], imgs[k][o], msks[k][v], msks[k][o], r, off, mg[v], mg[o], q["parent"])
            if not np.array_equal(g, q["out"]):
                fails.append(diff_report(tag, g, q["out"]))
        elif st == "smooth":
            g = ctx.smooth_constraint(q["inp"], mg[q["v"]])
            if not np.array_equal(g, q["out"]):
                fails.append(diff_report(tag, g, q["out"]))
        elif st == "order":
            g = ctx.order_constraint(q["inp"], mg[q["v"]])
            if not np.array_equal(g, q["out"]):
                fails.append(diff_report(tag, g, q["out"]))
        elif st == "uniq16":
            g0, g1 = ctx.uniqueness(q["inp"][0], q["inp"][1], mg[0], mg[1])
            if not np.array_equal(g0, q["out"][0]):
                fails.append(diff_report(tag + " d0", g0, q["out"][0]))
            if not np.array_equal(g1, q["out"][1]):
                fails.append(diff_report(tag + " d1", g1, q["out"][1]))
        elif st == "setb":
            v = q["v"]; o = 1 - v
            s, BL, BR = ctx.set_boundary_smooth(q["inp"], msks[k][v], mg[v], mg[o])
            assert s == 0
            # defined (and consumed by Rematch) only on masked pixels of the own margin
            YL, YR, XL, XR = mg[v][:4]
            sel = np.zeros(BL.shape, bool)
            sel[YL:YR + 1, XL:XR + 1] = msks[k][v][YL:YR + 1, XL:XR + 1] == 255
            if not np.array_equal(BL[sel], q["BL"][sel]):
                fails.append(diff_report(tag + " BL", np.where(sel, BL, 0), np.where(sel, q["BL"], 0)))
            if not np.array_equal(BR[sel], q["BR"][sel]):
                fails.append(diff_report(tag + " BR", np.where(sel, BR, 0), np.where(sel, q["BR"], 0)))
        elif st == "rematch":
            v = q["v"]; o = 1 - v
            s, g = ctx.rematch(imgs[k][v], imgs[k][o], msks[k][v], msks[k][o], r, mg[v], mg[o], q["inp"])
            assert s == 0
            if not np.array_equal(g, q["out"]):
                fails.append(diff_report(tag, g, q["out"]))
        elif st == "median":
            g = ctx.median_filter(q["inp"], msks[k][q["v"]], mg[q["v"]])
            if not np.array_equal(g, q["out"]):
                fails.append(diff_report(tag, g, q["out"]))
    assert not fails, "\n".join(fails[:12])


@pytest.mark.parametrize("name", list(CASES))
def test_fp64_stages(ctx, name):
    cfg, rec, fin = stages(name)
    imgs, msks = fin["imgs"], fin["msks"]
    worst = 0.0
    for q in rec:
        k, st = q["level"], q["stage"]
        mg = q["mg"]
        if st == "refine":
            v = q["v"]
            g = ctx.disparity_refine(q["inp"], imgs[k][v], imgs[k][1 - v], q["iters"], cfg.ws, mg[v])
            worst = max(worst, fp_close(g, q["out"]))
        elif st == "uniq64":
            g0, g1 = ctx.uniqueness(q["inp"][0], q["inp"][1], mg[0], mg[1])
            assert np.array_equal(g0, q["out"][0]), diff_report("uniq64 d0 L%d" % k, g0, q["out"][0])
            assert np.array_equal(g1, q["out"][1]), diff_report("uniq64 d1 L%d" % k, g1, q["out"][1])
    print("worst refine rel err", worst)


@pytest.mark.parametrize("name", list(CASES))
def test_cloud_and_erode(ctx, name):
    cfg, rec, fin = stages(name)
    k = cfg.pyr_levels - 1
    mg = fin["margin"]
    d0 = fin["disparity"][0]
    scale = cloud_scale(cfg)
    xo, bo = orc.disparity_to_cloud(d0, fin["msks"][k][0], fin["imgs"][k][0], cfg.Q, scale, cfg.R_final, cfg.T_final, mg[0])
    xg, bg = ctx.disparity_to_cloud(d0, fin["msks"][k][0], fin["imgs"][k][0], cfg.Q, scale, cfg.R_final, cfg.T_final, mg[0])
    assert xg.shape == xo.shape and len(xo) > 0
    assert np.array_equal(bg, bo)
    assert np.array_equal(np.isfinite(xg), np.isfinite(xo))  # d == 0 gives 1/0 in the reference too (.cpp:745)
    fin_ = np.isfinite(xo)
    assert np.array_equal(xg[fin_], xo[fin_]), np.abs(xg[fin_] - xo[fin_]).max()
    for ks in (3, 4, 7, 12):
        e = orc.erode_ellipse(fin["msks"][k][0], ks)
        g = ctx.erode_ellipse_is255(fin["msks"][k][0], ks)
        assert np.array_equal(g == 255, e == 255), "erode ksize %d" % ks


@pytest.mark.parametrize("name", list(CASES))
def test_full_pair_matches_oracle(ctx, name):
    cfg, rec, fin = stages(name)
    ref = orc.match_pair(cfg)
    res = ctx.match_pair(cfg)
    assert res.margin == ref["margin"]
    assert res.v_top == ref["v_top"]
    for v in range(2):
        # same staged oracle as the C whole-pair oracle
        assert np.array_equal(ref["disparity"][v], fin["disparity"][v])
        fp_close(res.disparity[v], ref["disparity"][v])
    assert res.n_points == ref["n_points"]
    assert np.array_equal(res.bgr, ref["bgr"])
    fin_ = np.isfinite(ref["xyz"])
    assert np.array_equal(np.isfinite(res.xyz), fin_)
    rel = np.abs(res.xyz[fin_] - ref["xyz"][fin_]) / np.maximum(1e-9, np.abs(ref["xyz"][fin_]))
    assert rel.max() < 1e-3  # north_star tolerance
    assert np.array_equal(res.xyz[fin_], ref["xyz"][fin_])


def test_pair_with_margins_unequal_in_height_and_width_matches_oracle(ctx):
    """The pair launches cover the larger margin of the two directions (margin_extent), rows and columns each: view 0's
    margin is 3 rows x 2 columns, view 1's 2 rows x 3 columns, so neither view's extent covers the other's.  The smallest
    pair the validator accepts (5 x 5, one level, radius 1); every output bit for bit."""
    cfg = synth.config_small(width=5, height=5, levels=1, radius=1, offset=2, pair=0, mask_kind="full", d0_l0=1.0, amp_l0=0.0)
    m0, m1 = np.zeros((5, 5), np.uint8), np.zeros((5, 5), np.uint8)
    m0[1:4, 1:3] = 255
    m1[1:3, 1:4] = 255
    cfg.mask = [m0, m1]
    ref = orc.match_pair(cfg)
    (yl0, yr0, xl0, xr0), (yl1, yr1, xl1, xr1) = ref["margin"][0][:4], ref["margin"][1][:4]
    assert yr0 - yl0 > yr1 - yl1 and xr0 - xl0 < xr1 - xl1
    assert all((ref["disparity"][v] != NOMATCH).any() for v in range(2)) and ref["n_points"] > 0
    res = ctx.match_pair(cfg)
    assert res.margin == ref["margin"]
    assert res.v_top == ref["v_top"]
    for v in range(2):
        assert np.array_equal(res.disparity[v], ref["disparity"][v]), diff_report("map %d" % v, res.disparity[v], ref["disparity"][v])
    assert res.n_points == ref["n_points"]
    assert np.array_equal(res.bgr, ref["bgr"])
    assert np.array_equal(res.xyz, ref["xyz"], equal_nan=True)


def test_run_is_deterministic_and_reusable(ctx):
    cfg = synth.config_small(**CASES["s128x96_r2_neg_holes"])
    a = ctx.match_pair(cfg)
    cfg2 = synth.config_small(**CASES["s96x64_r2"])
    ctx.match_pair(cfg2)  # different size in between: workspace is re-created
    b = ctx.match_pair(cfg)
    for v in range(2):
        assert np.array_equal(a.disparity[v], b.disparity[v])
    assert np.array_equal(a.xyz, b.xyz)


def test_degenerate_margin_is_an_error_not_exit(ctx):
    from reconstruction_amd import RsmError
    cfg = synth.config_small(**CASES["s96x64_r2"])
    cfg.mask = [np.zeros_like(cfg.mask[0]), np.zeros_like(cfg.mask[1])]
    with pytest.raises(RsmError) as e:
        ctx.match_pair(cfg)
    assert e.value.code == -2


# ---- adversarial stage inputs: random maps, far from what the pipeline would produce ----------------
def _rand_maps(seed, H=72, W=200, p_nomatch=0.3, lo=-4, hi=5):
    rng = np.random.default_rng(seed)
    d = rng.integers(lo, hi, size=(H, W)).astype(np.int16)
    d[rng.random((H, W)) < p_nomatch] = NOMATCH
    mask = np.where(rng.random((H, W)) < 0.85, 255, rng.integers(0, 255, size=(H, W))).astype(np.uint8)
    return d, mask


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random_inputs_constraint_stages(ctx, seed):
    rng = np.random.default_rng(100 + seed)
    H, W = 72, 200 + 7 * seed
    d0, m0 = _rand_maps(seed, H, W, p_nomatch=0.15 * seed)
    d1, m1 = _rand_maps(50 + seed, H, W, p_nomatch=0.2)
    r = 2
    XL = int(rng.integers(r, 12)); XR = W - 1 - int(rng.integers(r, 12))
    own = (r + seed, H - 1 - r - seed, XL, XR, XR - XL + 1, H - 2 * (r + seed))
    oth = (r, H - 1 - r, XL + 3, XR - 5, XR - XL - 7, H - 2 * r)
    for nm, fo, fg in [("smooth", orc.smooth_constraint, ctx.smooth_constraint),
                       ("order", orc.order_constraint, ctx.order_constraint)]:
        a, b = fg(d0, own), fo(d0, own)
        assert np.array_equal(a, b), diff_report("%s seed %d" % (nm, seed), a, b)
    a, b = ctx.median_filter(d0, m0, own), orc.median_filter(d0, m0, own)
    assert np.array_equal(a, b), diff_report("median", a, b)
    # uniqueness: disparities that actually point at each other some of the time
    p = d0.copy(); q = d1.copy()
    ys, xs = np.nonzero(p != NOMATCH)
    for y, x in list(zip(ys, xs))[::3]:
        t = x + int(p[y, x])
        if 0 <= t < W:
            q[y, t] = -p[y, x] + int(rng.integers(-2, 3))
    a, b = ctx.uniqueness_pass(p, q, own, oth), orc.uniqueness_pass(p, q, own, oth)
    assert np.array_equal(a, b), diff_report("uniq16 pass", a, b)
    pf = np.where(p == NOMATCH, float(NOMATCH), p + rng.normal(0, 0.4, p.shape))
    qf = np.where(q == NOMATCH, float(NOMATCH), q + rng.normal(0, 0.4, q.shape))
    a, b = ctx.uniqueness_pass(pf, qf, own, oth), orc.uniqueness_pass(pf, qf, own, oth)
    assert np.array_equal(a, b), diff_report("uniq64 pass", a, b)
    s1, BLg, BRg = ctx.set_boundary_smooth(d0, m0, own, oth)
    s2, BLo, BRo = orc.set_boundary_smooth(d0, m0, own, oth)
    assert s1 == s2 == 0
    sel = np.zeros((H, W), bool)
    sel[own[0]:own[1] + 1, own[2]:own[3] + 1] = m0[own[0]:own[1] + 1, own[2]:own[3] + 1] == 255
    assert np.array_equal(BLg[sel], BLo[sel]), diff_report("BL", np.where(sel, BLg, 0), np.where(sel, BLo, 0))
    assert np.array_equal(BRg[sel], BRo[sel]), diff_report("BR", np.where(sel, BRg, 0), np.where(sel, BRo, 0))


def test_order_constraint_heavy_crossings(ctx):
    rng = np.random.default_rng(7)
    H, W = 40, 300
    d = rng.integers(-30, 31, size=(H, W)).astype(np.int16)   # lots of crossings and ties
    d[rng.random((H, W)) < 0.5] = NOMATCH
    own = (2, H - 3, 2, W - 3, W - 4, H - 4)
    a, b = ctx.order_constraint(d, own), orc.order_constraint(d, own)
    assert np.array_equal(a, b), diff_report("order heavy", a, b)


def _pair_under_option(ctx, name, opt):
    cfg = synth.config_small(**CASES[name])
    base = ctx.match_pair(cfg)
    ctx.set_option(*opt)
    try:
        alt = ctx.match_pair(cfg)
    finally:
        ctx.set_option("ncc_bytes", 0)
    for v in range(2):
        assert np.array_equal(base.disparity[v], alt.disparity[v]), opt
    assert np.array_equal(base.xyz, alt.xyz, equal_nan=True)
    return base


@pytest.mark.parametrize("opt", [("ncc_bytes", 1)])
def test_kernel_variants_give_identical_results(ctx, opt):
    """The dot4 and the generic byte-wise NCC kernels are interchangeable bit for bit."""
    _pair_under_option(ctx, "s320x160_occluded_neg_r4", opt)


def test_ncc_bytes_option_changes_nothing_above_radius_7(ctx):
    """Radius 8 reaches the byte-wise kernel by dispatch; the option asks for what already happens."""
    base = _pair_under_option(ctx, "s192x128_r8", ("ncc_bytes", 1))
    assert base.n_points > 0


def test_reference_shaped_mirror_drives_the_pipeline(ctx):
    """StereoMatching.Init / MatchAllLayer (CStereoMatching.h:47-48) over the C ABI: same results as Context,
    bounds stored on the cameras (.cpp:27-28), InsertPoint called once per point in order, then filter."""
    from reconstruction_amd import Camera, ManageData, StereoMatching
    cfg = synth.config_small(**CASES["s128x96_r2_neg_holes"])
    top = 1 << (cfg.pyr_levels - 1)

    class Sink:
        def __init__(self):
            self.points, self.filtered = [], []

        def InsertPoint(self, p):
            self.points.append(np.array(p))

        def filter(self, idx):
            self.filtered.append(idx)

    data = ManageData(cam=[[Camera(camID=0, image=cfg.image[0], mask=cfg.mask[0]),
                            Camera(camID=1, image=cfg.image[1], mask=cfg.mask[1])]],
                      m_PyrmNum=cfg.pyr_levels, m_LowestLevelSize=(cfg.width // top, cfg.height // top),
                      m_OriginSize=(cfg.width, cfg.height),
                      rectified=[dict(Q=cfg.Q, R_final=cfg.R_final, T_final=cfg.T_final)])
    sink = Sink()
    sm = StereoMatching(0)
    sm.Init(data, sink, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    ref = ctx.match_pair(cfg)
    assert sm.margin == ref.margin and data.cam[0][0].bound == ref.margin[0] and data.cam[0][1].bound == ref.margin[1]
    assert np.array_equal(sm.disparity[0], ref.disparity[0])
    assert len(sink.points) == ref.n_points and sink.filtered == [0]
    assert np.array_equal(np.array(sink.points), ref.xyz, equal_nan=True)


def test_libm_exp_sensitivity(ctx):
    """Why the oracle and the kernels share one specified exp: switch the oracle to ANOTHER libm-grade exp (the host's expl
    rounded to double: differs from the specified one in 0.08 % of its last bits) and DisparityRefine, bit-identical
    otherwise, drifts -- agreement to ~1e-15 after 20 sweeps, up to ~2e-6 after the top level's 150; and against rounds 3-4's
    1-ulp-grade Taylor chain up to 7e-3.  Against the host libm's exp() call itself nothing drifts on a glibc / FMA host: the
    specification is that routine."""
    cfg, rec, fin = stages("s512x384_5levels")
    q = [r for r in rec if r["stage"] == "refine" and r["level"] == cfg.pyr_levels - 1][-1]
    k, v = q["level"], q["v"]
    g = ctx.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], q["iters"], cfg.ws, q["mg"][v])
    assert np.array_equal(g, q["out"])                      # specified exp on both sides: every bit
    try:
        orc.set_exp_mode(1)
        o_libm = orc.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], q["iters"], cfg.ws, q["mg"][v])
        orc.set_exp_mode(3)
        o_taylor = orc.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], q["iters"], cfg.ws, q["mg"][v])
        orc.set_exp_mode(2)
        o20 = orc.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], 20, cfg.ws, q["mg"][v])
        o = orc.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], q["iters"], cfg.ws, q["mg"][v])
    finally:
        orc.set_exp_mode(0)
    g20 = ctx.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], 20, cfg.ws, q["mg"][v])
    ok = o != NOMATCH
    e20 = np.abs(g20[ok] - o20[ok]) / np.maximum(1.0, np.abs(o20[ok]))
    e = np.abs(g[ok] - o[ok]) / np.maximum(1.0, np.abs(o[ok]))
    et = np.abs(g[ok] - o_taylor[ok]) / np.maximum(1.0, np.abs(o_taylor[ok]))
    print("expl-rounded exp: max rel after 20 sweeps %.2e, after %d sweeps %.2e (%d of %d pixels above 1e-9); Taylor-chain exp: %.2e"
          % (e20.max(), q["iters"], e.max(), int((e > 1e-9).sum()), int(ok.sum()), et.max()))
    assert e20.max() < 1e-12 and e.max() < 1e-4 and et.max() < 0.1
    assert np.array_equal(o_libm == NOMATCH, g == NOMATCH)
    if host_libm_is_glibc_with_fma():
        assert np.array_equal(g, o_libm)
    else:
        assert (np.abs(g[ok] - o_libm[ok]) / np.maximum(1.0, np.abs(o_libm[ok]))).max() < 1e-3


def test_whole_pair_against_the_libm_exp_oracle(ctx):
    """The honest statement of DisparityRefine parity.  Against the oracle with the SPECIFIED exp the HIP path is
    bit-identical (every other test).  The reference itself calls its C runtime's exp (.cpp:665-666); run the oracle
    that way (the host libm's exp() call) on the adversarial 5-level occluded pair on which rounds 1-4 had 7 pixels
    beyond 1e-3 (their exp was a 1-ulp-grade Taylor chain).  With the libm-grade specified exp north_star's bar holds
    AS STATED: identical NOMATCH sets and point count, no pixel above 1e-3 -- and on a glibc / FMA host, whose exp the
    specification restates, every bit of both maps and of the cloud is equal."""
    cfg, rec, fin = stages("s512x384_5levels")
    res = ctx.match_pair(cfg)
    orc.set_exp_mode(1)
    try:
        ref = orc.match_pair(cfg)
    finally:
        orc.set_exp_mode(0)
    st = libm_exp_stats(res.disparity, ref["disparity"])
    print("5-level 512x384 vs libm-exp oracle:", st)
    for s_ in st:
        assert s_["nomatch_mismatch"] == 0 and s_["above_1e3"] == 0 and s_["max_rel"] < 1e-4, s_
    assert res.n_points == ref["n_points"]
    if host_libm_is_glibc_with_fma():
        for v in range(2):
            assert np.array_equal(res.disparity[v], ref["disparity"][v])
        assert np.array_equal(res.xyz, ref["xyz"], equal_nan=True)


@pytest.mark.parametrize("T,first,rows,uw", [(2, 1, 0, 0), (3, 1, 7, 0), (4, 1, 16, 0), (3, 5, 0, 0), (4, 9, 33, 0), (2, 30, 12, 0), (3, 2, 1000, 0),
                                             (4, 22, 0, 0), (4, 1, 0, 56), (4, 2, 5, 56), (4, 3, 1000, 40), (4, 9, 33, 2), (2, 3, 9, 62), (3, 4, 11, 30), (4, 1, 17, 0)])
def test_refine_time_skewed_sweeps_are_bit_identical(ctx, T, first, rows, uw):
    """k_refine_skew (T Jacobi sweeps per launch: wave t of a workgroup streams down a strip of 64 lanes with sweep t on row
    s - 2t + 1, the state rings and both cache ways' rows in LDS, one 16-byte load and LDS write per wave and step, the common
    row straight-line with unscaled divisions and its guards looked at afterwards, cache updates deferred to the update list)
    from sweep `first` on -- from the first cached sweep, where nearly every pixel misses and every row takes the rare path, to
    the settled regime -- gives the single-sweep result, i.e. the oracle's, bit for bit; chunk heights from 4T rows to the whole
    level, sweep counts that leave 0..T-1 single sweeps at the end, strips of 66 - 2T columns (the default) and narrower."""
    with refine_options(ctx, refine_skew_from=first, refine_skew_T=T, refine_skew_min_px=0, refine_skew_rows=rows, refine_skew_uw=uw):
        for name in ("s512x384_5levels", "s192x128_ellipse", "s320x160_occluded_neg_r4"):
            cfg, rec, fin = stages(name)
            for q in rec:
                if q["stage"] != "refine":
                    continue
                k, v = q["level"], q["v"]
                for iters in (q["iters"], q["iters"] - 1):
                    want = q["out"] if iters == q["iters"] else orc.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], iters, cfg.ws, q["mg"][v])
                    g = ctx.disparity_refine(q["inp"], fin["imgs"][k][v], fin["imgs"][k][1 - v], iters, cfg.ws, q["mg"][v])
                    assert np.array_equal(g, want), diff_report("skew T %d from %d rows %d uw %d %s L%d v%d iters %d" % (T, first, rows, uw, name, k, v, iters), g, want)
            res = ctx.match_pair(cfg)
            for v in range(2):
                assert np.array_equal(res.disparity[v], fin["disparity"][v])


def wide_pair_config(height=64):
    """A one-level pair 12288 wide whose margins are 11048 columns: beyond the 10432 up to which OrderConstraint's row fits
    64 KB of LDS.  LowestLevelInitialMatch scores every masked pixel against every masked candidate of the other margin, so
    on the full mask the oracle needs minutes for a single row of this width; the masks keep 40 columns of every 256 (the
    margin is the masks' extent and stays as wide), with which the oracle takes about 10 s for the 48 margin rows."""
    cfg = synth.config_small(width=12288, height=height, levels=1, radius=2, offset=2, pair=0, mask_l0_width=11264, border_l0=8)
    m0, m1 = cfg.mask
    sh = int(np.nonzero(m1.any(axis=0))[0][0] - np.nonzero(m0.any(axis=0))[0][0])
    assert sh >= 0
    m0 = np.where((np.arange(cfg.width) % 256 < 40)[None, :], m0, 0).astype(np.uint8)
    m1 = np.zeros_like(m0)
    m1[:, sh:] = m0[:, :cfg.width - sh]
    cfg.mask = [m0, m1]
    return cfg


def test_wide_pair_beyond_64k_of_order_lds_matches_oracle(ctx):
    """The pair path (two directions per launch) on margin rows that need more than 64 KB of dynamic LDS in k_order: margins,
    both maps, point count, colours and XYZ bit for bit."""
    cfg = wide_pair_config()
    ref = orc.match_pair(cfg)
    for v in range(2):
        YL, YR, XL, XR = ref["margin"][v][:4]
        assert XR - XL + 1 > 10432 and YR - YL + 1 >= 40
        assert (ref["disparity"][v] != NOMATCH).sum() > 20000
    res = ctx.match_pair(cfg)
    assert res.margin == ref["margin"]
    assert res.v_top == ref["v_top"]
    for v in range(2):
        assert np.array_equal(res.disparity[v], ref["disparity"][v]), diff_report("wide pair map %d" % v, res.disparity[v], ref["disparity"][v])
    assert res.n_points == ref["n_points"] > 10000
    assert np.array_equal(res.bgr, ref["bgr"])
    assert np.array_equal(res.xyz, ref["xyz"], equal_nan=True)
