"""GPU seam levelling (csrc/k_meshstitch.hip) against the numpy restatement (tests/meshstitch_restatement.py, itself tested
in tests/test_meshstitch_cpu.py).  The fp64 state is exact: x, G, the degrees, the counts, the masks and the largest change are equal bit
for bit -- every step is the same IEEE operations in the same order, and G's terms are multiples of 1/2.  Only the relative residual, a
sum in another order, is compared to 1e-9.  If bits differ, look for a contracted multiply-add or another order of summation; the
comparison is not to be loosened."""
import ctypes as C

import numpy as np
import pytest
import torch

import meshcolor_restatement as mr
import meshstitch_restatement as ms
import meshstitch_scenes as sc
import poisson_restatement as pr
from reconstruction_amd import Camera, RsmError, synth
from test_gpu_meshcolor import EYE_P, K96, cam_pair, four_views, read_ply_mesh_color, sphere, sphere_camera

pytestmark = pytest.mark.gpu

KEYS_EXACT = ("n_vertices", "coloured", "incidences", "seam_incidences", "seam_two_terms", "seam_one_term", "seam_no_term", "dmax", "steps", "max_change",
              "clamped")
_cache = {}


def same_stats(got, want):
    return all(got[k] == want[k] for k in KEYS_EXACT) and abs(got["rel_residual"] - want["rel_residual"]) <= 1e-9 * want["rel_residual"]


def red_blue():
    Pa, _ = sphere_camera(0.0)
    Pb, _ = sphere_camera(180.0)
    red, blue = np.zeros((72, 96, 3), np.uint8), np.zeros((72, 96, 3), np.uint8)
    red[..., 2], blue[..., 0] = 255, 255
    return [cam_pair(Pa, red, None, Pb, blue, None)]


def restated(ctx, scene):
    """the restatement's colouring, visibility and whole call of a sphere scene, computed once: a dict that the tests only read"""
    if scene not in _cache:
        v, f, h = sphere(ctx)
        cams, min_cos = (four_views(), 0.2) if scene == "four" else (red_blue(), -0.99)
        views = mr.views_of(cams)
        c, best, cst = mr.color(v, f, views, 0, min_cos, 2.0 * h)
        vis, col = ms.visibility(v, f, views, min_cos, 2.0 * h)
        rgb, _, st, x = ms.stitch(v, f, views, min_cos, 2.0 * h, colouring=(c, best, cst, vis, col))
        _cache[scene] = dict(v=v, f=f, eps=2.0 * h, cams=cams, views=views, min_cos=min_cos, c=c, best=best, cst=cst, vis=vis, col=col, rgb=rgb, st=st, x=x)
    return _cache[scene]


# ---- 1: the solve stage ---------------------------------------------------------------------------------------------------------------------
def solve_cases():
    rng = np.random.default_rng(101)
    one = (np.zeros((0, 3), np.int32), np.int32([0]), np.uint8([[9, 200, 77]]), np.zeros((1, 3)))
    nv = 257                                                 # a soup over 257 vertices: more than one block, random valences
    f = rng.integers(0, nv, (700, 3)).astype(np.int32)
    best = rng.integers(-1, 3, nv).astype(np.int32)
    soup = (f, best, rng.integers(0, 256, (nv, 3)).astype(np.uint8), rng.integers(-300, 301, (nv, 3)) / 2.0)
    return dict(one=one, soup=soup, plane=sc.planted_plane()[:4])


@pytest.mark.parametrize("iterations", [1, 2, 50])
@pytest.mark.parametrize("case", ["one", "soup", "plane"])
def test_solve_stage_is_the_restatement_bit_for_bit(ctx, case, iterations):
    if "solve" not in _cache:
        _cache["solve"] = solve_cases()
    f, best, c, G = _cache["solve"][case]
    lam = 0.01
    want, wrel, inc = ms.solve(f, best, c, G, lam, iterations, return_inc=True)
    got, grel = ctx.mesh_stitch_solve(f, best, c, G, lam, iterations)
    diff = (got.view(np.uint64) != want.view(np.uint64)).sum()
    print("%s, %d steps: %d vertices, %d incidences, dmax %d; values whose bits differ: %d; residual %.6e (restated %.6e)"
          % (case, iterations, len(best), len(inc.I), inc.dmax, diff, grel, wrel))
    assert got.tobytes() == want.tobytes()
    assert abs(grel - wrel) <= 1e-9 * wrel
    cd = c.astype(np.float64)
    assert got[best < 0].tobytes() == cd[best < 0].tobytes()
    lonely = (inc.deg == 0) & (best >= 0) & (G == 0.0).all(axis=1)
    assert got[lonely].tobytes() == cd[lonely].tobytes()
    if case == "one":
        assert lonely.all() and grel == 0.0
    if case == "soup":                                       # the soup does have faces with a repeated index, and valences far apart
        assert ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum() > 0 and inc.dmax > 12 and (best < 0).sum() > 30
    if case == "plane":
        marks = sc.planted_plane()[4]
        assert lonely[marks["lone"]] and lonely[marks["loose"]] and inc.deg[marks["apex"]] == 2 and inc.dmax == 14   # the fin's ends: 12 + 2
        assert (got != cd).any()


def test_solve_stage_returns_a_seamless_colouring_unchanged(ctx):
    v, f, tex, best, c = sc.split_plane()
    one = np.zeros_like(best)
    G, deg, counts = ms.rhs(f, c, one)
    for steps in (0, 1, 64):
        x, rel = ctx.mesh_stitch_solve(f, one, c, G, 0.01, steps)
        assert x.tobytes() == c.astype(np.float64).tobytes() and rel == 0.0


# ---- 2: the visibility masks ----------------------------------------------------------------------------------------------------------------
def test_visibility_masks_equal_the_restatement(ctx):
    r = restated(ctx, "four")
    v, f, cams = r["v"], r["f"], r["cams"]
    assert sum(c.mask is None for pair in cams for c in pair) == 1 and any((c.mask != 255).any() for pair in cams for c in pair if c.mask is not None)
    got = ctx.mesh_visibility(v, f, cams, r["eps"])
    want = ms.masks_of(r["vis"])
    print("visibility: %d of %d masks differ; views per vertex %s" % ((got != want).sum(), len(v), np.bincount(r["vis"].sum(axis=0)).tolist()))
    assert got.tobytes() == want.tobytes()
    rgb, best, st = ctx.mesh_color(v, f, cams, r["eps"], mode=0)
    seen = best >= 0
    assert (((got[seen] >> best[seen].astype(np.uint64)) & np.uint64(1)) == 1).all() and (got[~seen] == 0).all()
    popcount = sum(int(((got >> np.uint64(k)) & np.uint64(1)).sum()) for k in range(64))
    assert popcount == st["visible_views"] == r["cst"]["visible_views"] and (got >> np.uint64(4)).max() == 0
    assert ms.vis_of(got, 4).tobytes() == r["vis"].tobytes()
    other = ctx.mesh_visibility(v, f, cams, 0.0, min_cos=0.6)
    assert other.tobytes() == ms.masks_of(ms.visibility(v, f, r["views"], 0.6, 0.0)[0]).tobytes() and (other != got).any()


# ---- 3: the right-hand side -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam_gradient", [True, False])
def test_rhs_stage_equals_the_restatement(ctx, seam_gradient):
    r = restated(ctx, "four")
    wG, wdeg, wcounts = ms.rhs(r["f"], r["c"], r["best"], r["vis"], r["col"], seam_gradient)
    full = ms.rhs(r["f"], r["c"], r["best"], r["vis"], r["col"], True)[2]
    assert min(full["seam_two_terms"], full["seam_one_term"], full["seam_no_term"]) > 50   # the scene has all three kinds
    G, deg, counts = ctx.mesh_stitch_rhs(r["v"], r["f"], r["cams"], r["c"], r["best"], ms.masks_of(r["vis"]), seam_gradient)
    print("seam_gradient %s: %s; G values that differ: %d, degrees that differ: %d" % (seam_gradient, counts, (G != wG).sum(), (deg != wdeg).sum()))
    assert G.tobytes() == wG.tobytes() and deg.tobytes() == wdeg.tobytes() and counts == wcounts
    assert (G.sum(axis=0) == 0.0).all() and (G != 0.0).any()


# ---- 4: the whole call ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["four", "redblue"])
def test_whole_call_equals_the_restatement(ctx, scene):
    r = restated(ctx, scene)
    v, f, cams = r["v"], r["f"], r["cams"]
    coloured = r["best"] >= 0
    frac = np.abs((r["x"] + 0.5) - np.round(r["x"] + 0.5))
    near_half = (frac < 1e-6) & coloured[:, None]            # a restated x within 1e-6 of a .5: its byte is not compared
    assert near_half.sum() < 1e-3 * near_half.size
    rgb, best, st = ctx.mesh_stitch(v, f, cams, r["eps"], min_cos=r["min_cos"])
    print("%s: %s; bytes that differ: %d (%d not compared); restated %s" % (scene, st, ((rgb != r["rgb"]) & ~near_half).sum(), near_half.sum(), r["st"]))
    assert ((rgb == r["rgb"]) | near_half).all()
    cbest = ctx.mesh_color(v, f, cams, r["eps"], mode=0, min_cos=r["min_cos"])[1]
    assert best.tobytes() == cbest.tobytes() == r["best"].tobytes()
    assert (rgb[~coloured] == 127).all() and (~coloured).sum() > 0
    assert same_stats(st, r["st"]) and st["steps"] <= 400 and st["seam_incidences"] > 0
    assert (rgb != r["c"]).any()
    if scene == "four":                                      # a given step count, and no seam gradient
        for kw in (dict(iterations=7), dict(seam_gradient=False, iterations=30, lam=0.05)):
            w = ms.stitch(v, f, r["views"], r["min_cos"], r["eps"], colouring=(r["c"], r["best"], r["cst"], r["vis"], r["col"]), **kw)
            g = ctx.mesh_stitch(v, f, cams, r["eps"], min_cos=r["min_cos"], **kw)
            assert g[0].tobytes() == w[0].tobytes() and same_stats(g[2], w[2]) and g[2]["steps"] == kw["iterations"]


# ---- 5: two constant images on a plane ------------------------------------------------------------------------------------------------------
def test_two_constant_images_on_a_plane_are_levelled_monotonically(ctx):
    nx, ny = 41, 31
    v, f = mr.grid_plane(nx, ny, -20.0, -15.0, 1.0, 0.0)    # the plane z = 0, normal +z; the cameras mirror each other in x = 0
    W, H = 96, 72
    ea, eb = np.array([-30.0, 0.0, 120.0]), np.array([30.0, 0.0, 120.0])
    Pa, Pb = mr.look_at(ea, (0, 0, 0), 200.0, 48.0, 36.0), mr.look_at(eb, (0, 0, 0), 200.0, 48.0, 36.0)
    ia, ib = np.full((H, W, 3), 100, np.uint8), np.full((H, W, 3), 140, np.uint8)
    cams = [cam_pair(Pa, ia, None, Pb, ib, None)]
    c, cbest, cst = ctx.mesh_color(v, f, cams, 0.5, mode=0)
    assert cst["coloured"] == len(v) and set(np.unique(c).tolist()) == {100, 140} and 0.4 < (cbest == 1).mean() < 0.6
    rgb, best, st = ctx.mesh_stitch(v, f, cams, 0.5)
    w = ms.stitch(v, f, mr.views_of(cams), 0.2, 0.5)
    assert rgb.tobytes() == w[0].tobytes() and same_stats(st, w[2]) and best.tobytes() == cbest.tobytes()
    assert st["seam_two_terms"] == st["seam_incidences"] > 0 and st["clamped"] == 0
    rows = rgb[:, 0].reshape(ny, nx).astype(int)
    print("row 15: %s" % rows[15].tolist())
    assert (rgb[:, 0] == rgb[:, 1]).all() and (rgb[:, 1] == rgb[:, 2]).all()
    assert rows.min() >= 100 and rows.max() <= 140 and (np.diff(rows, axis=1) >= 0).all()
    seam_jump = np.abs(np.diff(rows, axis=1)).max()
    assert seam_jump <= 2 and len(np.unique(rows)) > 10      # the step of 40 is spread over many columns
    assert abs(rgb.astype(np.float64).mean() - c.astype(np.float64).mean()) <= 0.5 + 1e-4 * 255.0   # the mean, to the bytes' rounding


# ---- 6: entry points, the empty mesh, refusals ----------------------------------------------------------------------------------------------
def test_host_device_and_last_entries_return_the_same_bytes(ctx):
    xyz, nrm = pr.sphere_samples(20000)
    v, f, pst = ctx.poisson_mesh(xyz, nrm, 5, trim_cells=0)  # the context's last mesh
    cams = four_views()
    eps = 2.0 * pst["h"]
    kw = dict(iterations=40)
    a = ctx.mesh_stitch(v, f, cams, eps, **kw)
    b = ctx.mesh_stitch(v, f, cams, eps, **kw)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[2]["coloured"] > 1000
    dv, df = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    drgb = torch.zeros((len(v), 3), dtype=torch.uint8, device="cuda")
    dbest = torch.zeros(len(v), dtype=torch.int32, device="cuda")
    st = ctx.mesh_stitch_device(dv.data_ptr(), len(v), df.data_ptr(), len(f), cams, drgb.data_ptr(), dbest.data_ptr(), eps, **kw)
    torch.cuda.synchronize()
    assert drgb.cpu().numpy().tobytes() == a[0].tobytes() and dbest.cpu().numpy().tobytes() == a[1].tobytes() and st == a[2]
    drgb.zero_()
    st = ctx.mesh_stitch_device(dv.data_ptr(), len(v), df.data_ptr(), len(f), cams, drgb.data_ptr(), 0, eps, **kw)   # best_view may be NULL
    torch.cuda.synchronize()
    assert st == a[2] and drgb.cpu().numpy().tobytes() == a[0].tobytes()
    c = ctx.mesh_stitch_last(cams, eps, **kw)
    assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes() and c[2] == a[2]
    rgb, best = np.zeros((len(v), 3), np.uint8), np.zeros(len(v), np.int32)
    ctx._chk(ctx._lib.rsm_mesh_last_colors(ctx._h, rgb.ctypes.data_as(C.c_void_p), best.ctypes.data_as(C.c_void_p)))
    assert rgb.tobytes() == a[0].tobytes() and best.tobytes() == a[1].tobytes()
    lv, lf = ctx.poisson_last_mesh(len(v), len(f))           # the mesh itself is untouched
    assert lv.tobytes() == v.tobytes() and lf.tobytes() == f.tobytes()
    ctx.mesh_clean_last(smooth_steps=1)                      # a new mesh has no colours until it is coloured
    with pytest.raises(RsmError) as e:
        ctx._chk(ctx._lib.rsm_mesh_last_colors(ctx._h, None, None))
    assert e.value.code == -5 and "colours" in str(e.value)


def test_the_empty_mesh_and_a_mesh_nobody_sees(ctx):
    cams = four_views()
    e = np.zeros((0, 3))
    rgb, best, st = ctx.mesh_stitch(e, e, cams, 1.0)
    assert rgb.shape == (0, 3) and best.shape == (0,) and st == ms.stitch(e, e, mr.views_of(cams), 0.2, 1.0)[2] and st["n_vertices"] == 0
    assert ctx.mesh_stitch(e, e, [], 1.0)[2]["steps"] == 0   # no views are needed for no vertices
    assert ctx.mesh_visibility(e, e, cams, 1.0).shape == (0,)
    v, f = mr.grid_plane(3, 3, 0.0, 0.0, 1.0, 5.0)
    rgb, best, st = ctx.mesh_stitch(v, e, cams, 1.0)         # vertices without faces: no normals, nothing coloured, the colouring's bytes
    assert (rgb == 127).all() and (best == -1).all() and st == ms.stitch(v, e, mr.views_of(cams), 0.2, 1.0)[2] and st["coloured"] == 0
    assert not ctx.mesh_visibility(v, e, cams, 1.0).any()


def test_invalid_input_is_refused_and_named(ctx):
    from reconstruction_amd._lib import RSM_E_INVALID, MeshColorParams, MeshStitchParams
    lib, h = ctx._lib, ctx._h
    v, f = mr.grid_plane(5, 5, -2.0, -2.0, 1.0, 10.0)
    f = np.ascontiguousarray(f[:, ::-1])                     # facing the camera: coloured, so that the solver's own refusal is reached
    img = np.zeros((72, 96, 3), np.uint8)
    P = K96 @ EYE_P
    good = [cam_pair(P, img, None, P, img, None)]
    rgb, best = np.zeros((len(v), 3), np.uint8), np.zeros(len(v), np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(V=v, F=f, cams=good, n_pairs=None, views="cams", params="p", sparams="sp", out=rgb, n_v=None, n_f=None, edit=None, **kw):
        p, sp = MeshColorParams(0, 0.2, 1.0), MeshStitchParams(0.01, 0, 1e-4, 1)
        for k, val in kw.items():
            setattr(p if k in ("mode", "min_cos", "depth_eps") else sp, "lambda" if k == "lam" else k, val)
        vw, keep = ctx.mesh_color_views(cams)
        if edit:
            edit(vw)
        st = lib.rsm_mesh_stitch(h, ptr(V), C.c_int64(len(V) if n_v is None else n_v), ptr(F), C.c_int64(len(F) if n_f is None else n_f),
                                 vw if views == "cams" else None, C.c_int(len(cams) if n_pairs is None else n_pairs),
                                 C.byref(p) if params == "p" else None, C.byref(sp) if sparams == "sp" else None, ptr(out), ptr(best), None)
        return st, (lib.rsm_last_error(h) or b"").decode()
    bad_i, neg_i, bad_c = f.copy(), f.copy(), v.copy()
    bad_i[7, 1] = len(v)
    neg_i[0, 0] = -1
    bad_c[3, 2] = np.nan
    sing = P.copy()
    sing[2, :3] = 2.0 * sing[0, :3]

    def set_field(name, val):
        return lambda vw: setattr(vw[0], name, val)

    def null_image(vw):
        vw[0].image[1] = None
    nan, inf = float("nan"), float("inf")
    for kw, name in ((dict(F=bad_i), "index"), (dict(F=neg_i), "index"), (dict(V=bad_c), "finite"),          # what rsm_mesh_color refuses ...
                     (dict(n_f=(2 ** 31 + 2) // 3), "nf"), (dict(n_f=-1), "nf"), (dict(n_v=-1), "nv"), (dict(n_v=2 ** 31), "nv"),
                     (dict(mode=2), "mode"), (dict(min_cos=1.0), "min_cos"), (dict(min_cos=nan), "min_cos"), (dict(depth_eps=-0.1), "depth_eps"),
                     (dict(depth_eps=inf), "depth_eps"), (dict(params=None), "params"), (dict(n_pairs=0), "n_pairs"),
                     (dict(views=None), "NULL"), (dict(V=None, n_v=len(v)), "NULL"), (dict(F=None, n_f=len(f)), "NULL"), (dict(out=None), "NULL"),
                     (dict(edit=null_image), "NULL"), (dict(edit=set_field("width", 0)), "width"), (dict(edit=set_field("height", -3)), "height"),
                     (dict(cams=[cam_pair(P, img, None, sing, img, None)]), "singular"),
                     (dict(mode=1), "mode 1 not 0"), (dict(cams=good * 33), "more than the 64"), (dict(sparams=None), "stitch params"),   # ... and its own
                     (dict(lam=0.0), "lambda"), (dict(lam=-1.0), "lambda"), (dict(lam=nan), "lambda"), (dict(lam=inf), "lambda"),
                     (dict(iterations=-1), "iterations"), (dict(iterations=1000001), "iterations"),
                     (dict(reduction=0.0), "reduction"), (dict(reduction=1.0), "reduction"), (dict(reduction=nan), "reduction"),
                     (dict(lam=1e-13, reduction=1e-4), "steps"),
                     (dict(seam_gradient=2), "seam_gradient"), (dict(seam_gradient=-1), "seam_gradient")):
        st, msg = call(**kw)
        assert st == RSM_E_INVALID and name in msg, (kw, st, msg)
    assert ctx.mesh_stitch(v, f, good, 1.0)[2]["coloured"] == len(v)
    assert call()[0] == 0 and call(cams=good * 32, iterations=3)[0] == 0 and call(iterations=5, reduction=7.0)[0] == 0   # (reduction is not used then)
    for fn in (lambda: ctx.mesh_stitch(v, neg_i, good, 1.0), lambda: ctx.mesh_stitch_last(good, 1.0, lam=0.0),
               lambda: ctx.mesh_stitch_device(0, len(v), 0, 0, good, 0, 0, 1.0), lambda: ctx.mesh_visibility(v, bad_i, good, 1.0),
               lambda: ctx.mesh_visibility(v, f, good * 33, 1.0), lambda: ctx.mesh_stitch_solve(bad_i, best, rgb, np.zeros((len(v), 3)), 0.01, 3),
               lambda: ctx.mesh_stitch_solve(f, best, rgb, np.zeros((len(v), 3)), 0.0, 3), lambda: ctx.mesh_stitch_solve(f, best, rgb, np.zeros((len(v), 3)), 0.01, -1),
               lambda: ctx.mesh_stitch_rhs(v, f, good, rgb, best + 2, np.zeros(len(v), np.uint64)),
               lambda: ctx.mesh_stitch_rhs(v, f, good, rgb, best - 2, np.zeros(len(v), np.uint64))):
        with pytest.raises(RsmError) as e:
            fn()
        assert e.value.code == RSM_E_INVALID


# ---- 7: the top of the stack ----------------------------------------------------------------------------------------------------------------
def test_cloud_optimization_run_mesh_clean_mesh_then_stitch_mesh(ctx):
    from reconstruction_amd import CloudOptimization, ManageData, StereoMatching
    # two odd pairs, as test_gpu_meshcolor.py's end-to-end test explains (synth's even pairs lie behind their own cameras)
    cfgs = [synth.config_small(320, 192, 3, radius=2, pair=5, mask_l0_width=70, border_l0=2, amp_l0=0.25),
            synth.config_small(320, 192, 3, radius=2, pair=7, mask_l0_width=70, border_l0=2, amp_l0=0.25, holes=True)]
    top = 1 << (cfgs[0].pyr_levels - 1)
    cams = []
    for c in cfgs:
        P0, P1, centre = synth.rectified_views(c.Q, c.R_final, c.T_final)
        cams.append([Camera(camID=0, image=c.image[0], mask=c.mask[0], CamCenter=centre, P=P0),
                     Camera(camID=1, image=c.image[1], mask=c.mask[1], CamCenter=centre, P=P1)])
    data = ManageData(cam=cams, m_PyrmNum=cfgs[0].pyr_levels, m_LowestLevelSize=(cfgs[0].width // top, cfgs[0].height // top),
                      m_OriginSize=(cfgs[0].width, cfgs[0].height), rectified=[dict(Q=c.Q, R_final=c.R_final, T_final=c.T_final) for c in cfgs])
    opt = CloudOptimization(ctx)
    opt.Init(100, 1, 50, 2, 40.0, data, False)
    sm = StereoMatching(0)
    sm.Init(data, opt, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    opt.run()
    with pytest.raises(ValueError, match="mesh"):
        opt.stitch_mesh()
    _, _, mst = opt.mesh(depth=7, trim_cells=2)
    v, f, _ = opt.clean_mesh()
    rgb, best, st = opt.stitch_mesh(iterations=60)
    assert opt.mesh_colors[0] is rgb and opt.mesh_result[0] is v
    w = ms.stitch(v, f, mr.views_of(cams), 0.2, 2.0 * mst["h"], iterations=60)
    print("run() -> mesh() -> clean_mesh() -> stitch_mesh(): %s" % st)
    assert rgb.tobytes() == w[0].tobytes() and best.tobytes() == w[1].tobytes() and same_stats(st, w[2])
    assert st["coloured"] > 0.5 * len(v) and st["seam_incidences"] > 0 and st["steps"] == 60
    c0 = opt.color_mesh(mode=0)                              # the colouring it started from
    assert c0[1].tobytes() == best.tobytes() and (c0[0] != rgb).any()
    cams[1][1].P = None                                      # pre-rectified input carries no P
    with pytest.raises(ValueError, match="pre-rectified input carries no P"):
        opt.stitch_mesh()


def test_cli_mesh_stitch_writes_the_stitched_mesh_to_outfilename(ctx, tmp_path, capsys):
    from PIL import Image
    from reconstruction_amd import StereoMatching
    from reconstruction_amd import config as cfgmod
    from reconstruction_amd.__main__ import main
    from test_gpu_meshcolor import _grid_step
    raw = synth.make_raw_pair(baseline=-150.0)
    root = str(tmp_path) + "/"
    (tmp_path / "mask").mkdir()
    for j in range(2):
        Image.fromarray(raw["image"][j][:, :, ::-1]).save(root + "0001_Cam%d.png" % j)
        Image.fromarray(raw["mask"][j]).save(root + "mask/0001_Cam%d.png" % j)
    cfgmod.dump_opencv_yaml(root + "calib_camera.yml", {"intrinsic-0": raw["K"][0], "extrinsic-0": raw["E"][0],
                                                         "intrinsic-1": raw["K"][1], "extrinsic-1": raw["E"][1]})
    cfgmod.dump_opencv_yaml(root + "config.yml", {
        "filepath": root, "outfilename": root + "out", "isoutput": 0, "camera_calib_name": "calib_camera.yml",
        "PyrmNum": raw["pyr_levels"], "LowestLevelWidth": raw["lowest"][0], "LowestLevelHeight": raw["lowest"][1],
        "imagelist": ["0001_Cam%d.png" % j for j in range(2)], "masklist": ["mask\\0001_Cam%d.png" % j for j in range(2)],
        "camID": np.array([[0, 1]], np.uint8)})
    base = [root + "config.yml", "--mls-radius", "10", "--mesh-depth", "7", "--mesh-clean"]
    # --mesh-stitch alone implies --mesh-color; --mesh-color-mode is not consulted
    assert main(base + ["--mesh-stitch", "--mesh-color-mode", "blend", "--mesh-stitch-lambda", "0.02", "--mesh-stitch-iterations", "50"]) == 0
    out = capsys.readouterr().out.splitlines()
    v, f, rgb = read_ply_mesh_color(root + "out.ply")
    mv, mf = pr.read_ply_mesh(root + "bigmesh.ply")
    assert v.tobytes() == mv.tobytes() and np.array_equal(f, mf) and open(root + "out_cloud.ply", "rb").read().startswith(b"ply")
    data, _ = cfgmod.load_config(root + "config.yml")
    sm = StereoMatching(0)
    sm.Init(data, None, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    h = _grid_step(ctx, root)
    want, wbest, wst, _ = ms.stitch(mv, mf, mr.views_of(data.cam), 0.2, 2.0 * h, lam=0.02, iterations=50)
    assert rgb.tobytes() == want.tobytes() and wst["coloured"] > 0
    assert out[-1].startswith("Mesh stitch: %d of %d vertices coloured from 2 views, %d of %d incidences across a seam, 50 steps"
                              % (wst["coloured"], len(mv), wst["seam_incidences"], wst["incidences"])) and out[-1].endswith("-> %sout.ply" % root)
    assert not any(l.startswith("Mesh colour:") for l in out)
    assert main(base + ["--mesh-stitch", "--mesh-stitch-lambda", "0"]) == 1
    assert "lambda" in capsys.readouterr().out
