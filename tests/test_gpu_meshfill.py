"""GPU colour fill (csrc/k_meshfill.hip) against the numpy restatement (tests/meshfill_restatement.py, itself tested in
tests/test_meshfill_cpu.py).  The fp64 state is exact: the front's values and levels, x after any number of steps, the bytes and every
stat are equal bit for bit -- every sum is the same IEEE operations in the same order.  If bits differ, look for a contracted multiply-add
or another order of summation; the comparison is not to be loosened."""
import ctypes as C

import numpy as np
import pytest
import torch

import meshfill_restatement as mf
import meshfill_scenes as fs
import poisson_restatement as pr
from reconstruction_amd import Camera, RsmError, synth
from test_gpu_meshcolor import four_views, read_ply_mesh_color, sphere

pytestmark = pytest.mark.gpu

BATCH = 16                                                   # RSM_MESH_FILL_ROUND_BATCH (include/rsm.h): the rounds between two read-backs
_cache = {}


def front_cases():
    """name -> (f, rgb, best, max_rounds)"""
    if "front" not in _cache:
        cases = {k: fs.fixture(k) for k in fs.EXACT_FIXTURES}
        e = np.zeros((0, 3), np.int32)
        cases["one_unknown"] = (e, np.uint8([[127, 127, 127]]), np.int32([-1]), 0)
        cases["one_known"] = (e, np.uint8([[9, 200, 77]]), np.int32([3]), 0)
        cases["soup256"] = fs.soup(256) + (0,)
        cases["planted"] = fs.planted()[:3] + (0,)
        cases["hub"] = fs.hub() + (0,)
        for L in (BATCH - 1, BATCH, BATCH + 1):
            cases["strip_L%d" % L] = fs.strip_of_rounds(L) + (0,)
        cases["left_columns_cap1"] = fs.plane_left_columns() + (1,)
        cases["left_columns_cap2"] = fs.plane_left_columns() + (2,)
        _cache["front"] = cases
    return _cache["front"]


FRONT_NAMES = sorted(fs.EXACT_FIXTURES) + ["one_unknown", "one_known", "soup256", "planted", "hub", "strip_L15", "strip_L16", "strip_L17", "left_columns_cap1",
                                          "left_columns_cap2"]


def restated_front(name):
    key = "front:" + name
    if key not in _cache:
        f, rgb, best, cap = front_cases()[name]
        _cache[key] = mf.front(f, rgb, best, cap)
    return _cache[key]


def restated_fill(name):
    key = "fill:" + name
    if key not in _cache:
        f, rgb, best, cap = front_cases()[name]
        _cache[key] = mf.fill(f, rgb, best, cap)
    return _cache[key]


# ---- 1: the front stage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FRONT_NAMES)
def test_front_stage_is_the_restatement_bit_for_bit(ctx, name):
    f, rgb, best, cap = front_cases()[name]
    wx, wlevel, wL = restated_front(name)
    x, level, L = ctx.mesh_fill_front(f, rgb, best, cap)
    print("%s: %d vertices, %d unknown, L %d (restated %d); values whose bits differ: %d, levels that differ: %d"
          % (name, len(best), (best < 0).sum(), L, wL, (x.view(np.uint64) != wx.view(np.uint64)).sum(), (level != wlevel).sum()))
    assert L == wL and level.tobytes() == wlevel.tobytes() and x.tobytes() == wx.tobytes()
    untouched = level <= 0
    assert x[untouched].tobytes() == rgb.astype(np.float64)[untouched].tobytes()
    if name.startswith("strip_L"):
        assert L == int(name[7:]) and (level >= 0).all()
    if name == "hub":
        assert L == 2 and level[0] == 1 and mf.all_incidences(f, len(best)).deg[0] == 2000
    if name == "planted":
        marks = fs.planted()[3]
        assert (level[[marks["loose_unknown"], *marks["island"]]] == -1).all() and level[marks["apex"]] == 0
    if cap:
        assert L == cap and (level == -1).any()
    if name in ("soup256", "soup257"):
        assert len(best) == int(name[4:]) and ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum() > 0


def test_front_does_not_depend_on_the_round_batch(ctx):
    for name in ("strip_L15", "strip_L16", "strip_L17", "left_columns", "disc10_cap3"):
        f, rgb, best, cap = front_cases()[name]
        wx, wlevel, wL = restated_front(name)
        for batch in (1, 3, 16, 1024):
            x, level, L = ctx.mesh_fill_front(f, rgb, best, cap, round_batch=batch)
            assert L == wL and level.tobytes() == wlevel.tobytes() and x.tobytes() == wx.tobytes(), (name, batch)


# ---- 2: the solve stage -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 50])
@pytest.mark.parametrize("name", ["soup257", "disc8", "strip200", "disc10_cap3"])
def test_solve_stage_is_the_restatement_bit_for_bit(ctx, name, iterations):
    f, rgb, best, cap = front_cases()[name]
    x0, level, L = restated_front(name)
    want = mf.solve(f, x0, level, L, iterations)
    got = ctx.mesh_fill_solve(f, x0, level, L, iterations)
    print("%s, %d steps: L %d; values whose bits differ: %d" % (name, iterations, L, (got.view(np.uint64) != want.view(np.uint64)).sum()))
    assert got.tobytes() == want.tobytes()
    filled = level >= 1
    assert got[~filled].tobytes() == x0[~filled].tobytes() and (got[filled] != x0[filled]).any()
    assert ctx.mesh_fill_solve(f, x0, level, L, 0).tobytes() == x0.tobytes()


# ---- 3: the whole call ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fs.EXACT_FIXTURES) + ["planted", "hub", "one_unknown", "one_known"])
def test_whole_call_equals_the_restatement(ctx, name):
    f, rgb, best, cap = front_cases()[name]
    wout, wlevel, wst, wx, _ = restated_fill(name)
    out, level, st = ctx.mesh_fill_colors(f, rgb, best, max_rounds=cap)
    print("%s: %s; bytes that differ: %d; restated %s" % (name, st, (out != wout).sum(), wst))
    assert out.tobytes() == wout.tobytes() and level.tobytes() == wlevel.tobytes()
    assert st == wst
    known = best >= 0
    assert out[known].tobytes() == rgb[known].tobytes() and out[level < 0].tobytes() == rgb[level < 0].tobytes()
    if name in fs.EXACT_FIXTURES:
        assert st["filled"] > 0 and (out[level >= 1] != 127).any()
    if name == "soup257":                                    # a given step count
        g, w = ctx.mesh_fill_colors(f, rgb, best, iterations=7), mf.fill(f, rgb, best, iterations=7)
        assert g[0].tobytes() == w[0].tobytes() and g[2] == w[2] and g[2]["steps"] == 7


def test_no_unknown_and_no_known_vertex_give_the_input_s_bytes(ctx):
    f, rgb, best = fs.soup()
    for b in (np.zeros_like(best), np.full_like(best, -1)):
        out, level, st = ctx.mesh_fill_colors(f, rgb, b)
        w = mf.fill(f, rgb, b)
        assert out.tobytes() == rgb.tobytes() and level.tobytes() == w[1].tobytes() and st == w[2] and st["filled"] == st["steps"] == 0
    e = np.zeros((0, 3), np.int32)
    out, level, st = ctx.mesh_fill_colors(e, np.zeros((0, 3), np.uint8), np.zeros(0, np.int32))
    assert out.shape == (0, 3) and level.shape == (0,) and st == mf.fill(e, np.zeros((0, 3), np.uint8), np.zeros(0, np.int32))[2]


def test_host_device_and_last_entries_agree(ctx):
    v, f, h = sphere(ctx)
    cams = four_views()
    xyz, nrm = pr.sphere_samples(20000)
    lv, lf, _ = ctx.poisson_mesh(xyz, nrm, 5, trim_cells=0)  # the context's last mesh: the same sphere
    assert lv.tobytes() == v.tobytes() and lf.tobytes() == f.tobytes()
    with pytest.raises(RsmError) as e:                       # a mesh without colours
        ctx.mesh_fill_colors_last()
    assert e.value.code == -5 and "colours" in str(e.value)
    for how in ("color", "stitch"):
        if how == "color":
            c, best, cst = ctx.mesh_color_last(cams, 2.0 * h, mode=0)
        else:
            c, best, cst = ctx.mesh_stitch_last(cams, 2.0 * h, iterations=40)
        grey = best < 0
        assert 0 < grey.sum() < len(v) - 1000 and (c[grey] == 127).all()
        want, wlevel, wst, _, _ = mf.fill(f, c, best)
        a, alevel, ast = ctx.mesh_fill_colors(f, c, best)
        assert a.tobytes() == want.tobytes() and alevel.tobytes() == wlevel.tobytes() and ast == wst
        assert wst["unreached"] == 0 and wst["filled"] == grey.sum()   # the sphere is connected: nothing stays as it was
        df = torch.from_numpy(f).cuda()
        drgb, dbest = torch.from_numpy(c).cuda(), torch.from_numpy(best).cuda()
        dlevel = torch.zeros(len(v), dtype=torch.int32, device="cuda")
        st = ctx.mesh_fill_colors_device(df.data_ptr(), len(v), len(f), drgb.data_ptr(), dbest.data_ptr(), dlevel.data_ptr())
        torch.cuda.synchronize()
        assert drgb.cpu().numpy().tobytes() == a.tobytes() and dlevel.cpu().numpy().tobytes() == alevel.tobytes() and st == ast
        assert dbest.cpu().numpy().tobytes() == best.tobytes()
        drgb = torch.from_numpy(c).cuda()
        st = ctx.mesh_fill_colors_device(df.data_ptr(), len(v), len(f), drgb.data_ptr(), dbest.data_ptr())   # level may be NULL
        torch.cuda.synchronize()
        assert drgb.cpu().numpy().tobytes() == a.tobytes() and st == ast
        l_rgb, l_best, l_st = ctx.mesh_fill_colors_last()
        assert l_rgb.tobytes() == a.tobytes() and l_best.tobytes() == best.tobytes() and l_st == ast
        rgb2, best2 = np.zeros((len(v), 3), np.uint8), np.zeros(len(v), np.int32)
        ctx._chk(ctx._lib.rsm_mesh_last_colors(ctx._h, rgb2.ctypes.data_as(C.c_void_p), best2.ctypes.data_as(C.c_void_p)))
        assert rgb2.tobytes() == a.tobytes() and best2.tobytes() == best.tobytes()
        again = ctx.mesh_fill_colors_last()                  # the filled vertices keep best_view -1: the same bytes again
        assert again[0].tobytes() == a.tobytes() and again[2] == ast
    lv, lf = ctx.poisson_last_mesh(len(v), len(f))           # the mesh itself is untouched
    assert lv.tobytes() == v.tobytes() and lf.tobytes() == f.tobytes()
    ctx.mesh_clean_last(smooth_steps=1)                      # a new mesh has no colours until it is coloured
    with pytest.raises(RsmError) as e:
        ctx.mesh_fill_colors_last()
    assert e.value.code == -5


def test_invalid_input_is_refused_and_named(ctx):
    from reconstruction_amd._lib import RSM_E_INVALID, MeshFillParams
    lib, h = ctx._lib, ctx._h
    f, rgb, best = fs.strip(40)
    n = len(best)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(F=f, c=rgb, b=best, params="p", n_v=None, n_f=None, **kw):
        n, nf = (0 if b is None else len(b)) or len(best), (0 if F is None else len(F)) or len(f)
        p = MeshFillParams(0, 0, 1e-4)
        for k, val in kw.items():
            setattr(p, k, val)
        out = None if c is None else c.copy()
        st = lib.rsm_mesh_fill_colors(h, ptr(F), C.c_int64(n if n_v is None else n_v), C.c_int64(nf if n_f is None else n_f), ptr(out), ptr(b), None,
                                      C.byref(p) if params == "p" else None, None)
        return st, (lib.rsm_last_error(h) or b"").decode()
    bad_i, neg_i = f.copy(), f.copy()
    bad_i[7, 1] = n
    neg_i[0, 0] = -1
    nan = float("nan")
    deep = fs.strip_of_rounds(1100)
    for kw, name in ((dict(F=bad_i), "index"), (dict(F=neg_i), "index"), (dict(n_f=(2 ** 31 + 2) // 3), "nf"), (dict(n_f=-1), "nf"), (dict(n_v=-1), "nv"),
                     (dict(n_v=2 ** 31), "nv"), (dict(F=None), "NULL"), (dict(c=None), "NULL"), (dict(b=None), "NULL"), (dict(params=None), "params"),
                     (dict(max_rounds=-1), "max_rounds"), (dict(iterations=-1), "iterations"), (dict(iterations=1000001), "iterations"),
                     (dict(reduction=0.0), "reduction"), (dict(reduction=1.0), "reduction"), (dict(reduction=nan), "reduction"),
                     (dict(F=deep[0], c=deep[1], b=deep[2], reduction=1e-300), "steps")):   # 977 (L + 1) steps at that reduction
        st, msg = call(**kw)
        assert st == RSM_E_INVALID and msg.startswith("mesh_fill") and name in msg, (kw, st, msg)
    assert call()[0] == 0 and call(iterations=5, reduction=7.0)[0] == 0 and call(max_rounds=2)[0] == 0   # (reduction is not used then)
    x = np.zeros((n, 3))
    for fn in (lambda: ctx.mesh_fill_colors(neg_i, rgb, best), lambda: ctx.mesh_fill_colors(f, rgb, best, max_rounds=-2),
               lambda: ctx.mesh_fill_colors_device(0, n, len(f), 0, 0), lambda: ctx.mesh_fill_colors_last(iterations=-1),
               lambda: ctx.mesh_fill_front(bad_i, rgb, best), lambda: ctx.mesh_fill_front(f, rgb, best, -1),
               lambda: ctx.mesh_fill_solve(bad_i, x, best, 3, 3), lambda: ctx.mesh_fill_solve(f, x, best, -1, 3), lambda: ctx.mesh_fill_solve(f, x, best, 3, -1),
               lambda: ctx.mesh_fill_solve(f, x, best, 3, 1000001)):
        with pytest.raises(RsmError) as e:
            fn()
        assert e.value.code == RSM_E_INVALID
    for batch in (-1, 1025):
        with pytest.raises(RsmError) as e:
            ctx.mesh_fill_front(f, rgb, best, round_batch=batch)
        assert e.value.code == RSM_E_INVALID and "round_batch" in str(e.value)


# ---- 4: the top of the stack ------------------------------------------------------------------------------------------------------------------
def test_cloud_optimization_stitch_mesh_then_fill_mesh_colors(ctx):
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
    opt.mesh(depth=7, trim_cells=2)
    v, f, _ = opt.clean_mesh()
    with pytest.raises(ValueError, match="color_mesh"):
        opt.fill_mesh_colors()
    c, cbest, sst = opt.stitch_mesh(iterations=60)
    grey = cbest < 0
    assert grey.sum() > 0 and (c[grey] == 127).all()
    rgb, best, st = opt.fill_mesh_colors()
    assert opt.mesh_colors[0] is rgb
    want, wlevel, wst, _, _ = mf.fill(f, c, cbest)
    print("run() -> mesh() -> clean_mesh() -> stitch_mesh() -> fill_mesh_colors(): %s" % st)
    assert rgb.tobytes() == want.tobytes() and best.tobytes() == cbest.tobytes() and st == wst
    assert rgb[~grey].tobytes() == c[~grey].tobytes()
    # the cleaned surface is one piece: every vertex no view saw is filled, none stays grey
    assert (wlevel >= 0).all() and st["unreached"] == 0 and st["filled"] == grey.sum() and (rgb[grey] != 127).any()
    capped = opt.fill_mesh_colors(max_rounds=1)             # (on the filled colours: best_view still tells the filled vertices apart)
    assert capped[2]["rounds"] == 1 and capped[2]["known"] == st["known"]


def test_cli_mesh_color_fill_writes_the_filled_mesh_to_outfilename(ctx, tmp_path, capsys):
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
    # --mesh-color-fill alone implies --mesh-color; with --mesh-stitch it runs after it
    assert main(base + ["--mesh-stitch", "--mesh-stitch-iterations", "50", "--mesh-color-fill"]) == 0
    out = capsys.readouterr().out.splitlines()
    v, f, rgb = read_ply_mesh_color(root + "out.ply")
    mv, mf_ = pr.read_ply_mesh(root + "bigmesh.ply")
    assert v.tobytes() == mv.tobytes() and np.array_equal(f, mf_)
    data, _ = cfgmod.load_config(root + "config.yml")
    sm = StereoMatching(0)
    sm.Init(data, None, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    eps = 2.0 * _grid_step(ctx, root)
    c, best, _ = ctx.mesh_stitch(mv, mf_, data.cam, eps, iterations=50)   # (held to its own restatement in test_gpu_meshstitch.py)
    want, wlevel, wst, _, _ = mf.fill(mf_, c, best)
    assert (best < 0).sum() > 0 and wst["filled"] > 0 and rgb.tobytes() == want.tobytes() and (rgb != c).any()
    assert out[-2].startswith("Mesh stitch: ") and out[-1].startswith("Mesh colour fill: %d of %d uncoloured vertices filled in %d rounds, %d left as they were, %d steps"
                                                                       % (wst["filled"], wst["filled"] + wst["unreached"], wst["rounds"], wst["unreached"], wst["steps"]))
    assert out[-1].endswith("-> %sout.ply" % root)
    assert main(base + ["--mesh-color-fill", "2"]) == 0       # bare --mesh-color-fill implies --mesh-color (the blend), ROUNDS caps the front
    out = capsys.readouterr().out.splitlines()
    assert out[-2].startswith("Mesh colour: ") and (" in 2 rounds, " in out[-1] or " in 1 rounds, " in out[-1])
    assert main(base + ["--mesh-color-fill", "-1"]) == 1
    assert "max_rounds" in capsys.readouterr().out
