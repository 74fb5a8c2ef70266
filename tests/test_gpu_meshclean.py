"""GPU mesh smoothing and clean-up (csrc/k_meshclean.hip) against the numpy restatement
(tests/meshclean_restatement.py).  Everything is exact: smoothed positions are the same bits (every operation is an IEEE basic operation in
a fixed order), labels, faces, counts and the two fp64 figures of the statistics are equal.  If the bits differ, look for a contracted
multiply-add or another order of summation; the comparison is not to be loosened.

Figures (MI355X; noisy sphere, five cotangent steps; GPU and restatement agree bit for bit, 0 coordinates differ in all 32 smoothing cases):
  depth 5   max radial error 0.2892 h -> 0.0846 h   mean 0.0358 h -> 0.0291 h
  depth 6   max radial error 0.2721 h -> 0.0567 h   mean 0.0313 h -> 0.0168 h
  run() -> mesh(depth 7, trim 4) -> clean_mesh(): 13 296 faces -> 12 756, 3 of 5 pieces removed (540 faces), no border vertex."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import meshclean_restatement as mr
import poisson_restatement as pr
from reconstruction_amd import synth

pytestmark = pytest.mark.gpu

CLOSED = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0, edge_without_opposite=0, edges_not_in_two_faces=0, euler=2,
              unused_vertices=0)
_cache = {}


def gpu_mesh(ctx, depth, n, cap=False, trim=0):
    """the GPU's own Poisson mesh of the sphere / cap samples (cached per session): (vertices, faces, h)"""
    key = (depth, n, cap, trim)
    if key not in _cache:
        xyz, nrm = pr.sphere_samples(n, cap=cap)
        v, f, st = ctx.poisson_mesh(xyz, nrm, depth, trim_cells=trim)
        _cache[key] = (v, f, st["h"])
    return _cache[key]


def sliver_mesh():
    """a small open mesh holding an obtuse sliver (a negative cotangent to clamp), a zero-area face (collinear: n2 = 0, weight 0), a face
    with a repeated index, and an interior vertex (4) whose corner list meets all of them"""
    v = np.float32([[0, 0, 0], [4, 0, 0], [8, 0, 0], [0, 3, 0.5], [3, 0.01, 0.25], [8, 3, 0], [4, 6, 1], [2, 0, 0], [4, -5, 0.5]])
    f = np.int32([[0, 7, 4], [7, 1, 4], [1, 2, 4], [2, 5, 4], [5, 6, 4], [6, 3, 4], [3, 0, 4],     # a fan round 4: (0, 7, 4), (7, 1, 4), (1, 2, 4) are slivers
                  [0, 1, 7],                                                                        # collinear: zero area
                  [4, 4, 6],                                                                        # a repeated index
                  [0, 8, 1], [1, 8, 2]])
    return v, f


# ---- 1: smoothing, the same bits --------------------------------------------------------------------------------------------------------
def check_smoothing(ctx, v, f, want_border=None):
    _, border = mr.incidences(f, len(v))
    if want_border is not None:
        assert int(border.sum()) == want_border
    for steps in (1, 5):
        for cot in (False, True):
            for bnd in (False, True):
                got, nb = ctx.mesh_smooth(v, f, steps, cot, bnd, return_border=True)
                want = mr.smooth(v, f, steps, cot, bnd)
                diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
                print("steps %d cotangent %d boundary %d: %d vertices, %d border, coordinates whose bits differ: %d" % (steps, cot, bnd, len(v), nb, diff))
                assert nb == int(border.sum())
                assert got.tobytes() == want.tobytes()
    return got


@pytest.mark.parametrize("depth,n", [(5, 20000), (6, 80000)])
def test_smoothing_of_the_closed_sphere_is_the_restatements_bits(ctx, depth, n):
    v, f, h = gpu_mesh(ctx, depth, n)
    got = check_smoothing(ctx, v, f, want_border=0)
    assert pr.manifold_report(got, f) == CLOSED                   # connectivity is untouched: the smoothed sphere is still closed
    # the faces as the library hands them back after smoothing (nothing to remove on the sphere): unchanged, with the smoothed positions
    v2, f2, s2 = ctx.mesh_clean(v, f, smooth_steps=5, min_piece=0.0)
    assert np.array_equal(f2, f) and v2.tobytes() == got.tobytes() and s2["n_faces"] == len(f) and s2["vertices_dropped"] == 0
    assert not np.array_equal(got, v)


def test_smoothing_of_the_trimmed_cap_is_the_restatements_bits(ctx):
    v, f, h = gpu_mesh(ctx, 5, 20000, cap=True, trim=2)
    check_smoothing(ctx, v, f, want_border=179)
    _, border = mr.incidences(f, len(v))
    fixed = ctx.mesh_smooth(v, f, 5, True, False)
    assert np.array_equal(fixed[border], v[border]) and not np.array_equal(fixed[~border], v[~border])


def test_smoothing_with_a_sliver_and_a_zero_area_face_is_the_restatements_bits(ctx):
    v, f = sliver_mesh()
    P = v.astype(np.float64)
    assert mr.corner_n2(P[[0]], P[[1]], P[[7]])[0][0] == 0.0                            # the collinear face
    n2, dot = mr.corner_n2(P[[4]], P[[7]], P[[1]])                                      # the sliver's obtuse corner at vertex 4
    assert n2[0] > 0.0 and dot[0] < 0.0
    got = check_smoothing(ctx, v, f)
    assert np.isfinite(got).all()


# ---- 2: component labels ------------------------------------------------------------------------------------------------------------------
def pieces_mesh():
    """a grid, a second grid that touches it at ONE shared vertex only, a fan far away whose faces are split round the others, a repeated index"""
    v1, f1 = mr.grid_mesh(40, 30)
    v2, f2 = mr.grid_mesh(25, 35)
    v2 = v2 + np.float32([39.0, 29.0, 0.0])
    f2 = f2 + len(v1)
    f2[f2 == len(v1)] = len(v1) - 1
    v3, f3 = mr.fan_mesh(50)
    v3 = v3 + np.float32([200.0, 0.0, 0.0])
    f3 = f3 + len(v1) + len(v2)
    return np.concatenate([v1, v2, v3]), np.concatenate([f3[:20], f1, [[0, 0, 1]], f2, f3[20:]]).astype(np.int32)


def test_component_labels_are_the_lowest_face_of_each_piece(ctx):
    v, f = pieces_mesh()
    want, n = mr.components(f)
    got, ng = ctx.mesh_components(f, len(v))
    assert n == ng == 3 and np.array_equal(got, want)
    assert (got == -1).sum() == 1 and sorted(set(got.tolist())) == [-1, 0, 20, 20 + 2 * 39 * 29 + 1]
    # the two grids share a vertex and nothing else: separate pieces
    i1, i2 = 20, 20 + 2 * 39 * 29 + 1
    assert (f[i1:i2 - 1] == 40 * 30 - 1).any() and (f[i2:i2 + 2 * 24 * 34] == 40 * 30 - 1).any() and got[i1] != got[i2]
    # shuffled faces: the labels are still the lowest index of each piece
    rng = np.random.default_rng(3)
    fs = f[rng.permutation(len(f))]
    assert np.array_equal(ctx.mesh_components(fs, len(v))[0], mr.components(fs)[0])
    # one large piece
    sv, sf, _ = gpu_mesh(ctx, 6, 80000)
    lab, n = ctx.mesh_components(sf, len(sv))
    assert n == 1 and (lab == 0).all()


# ---- 3: the constructed fixture -----------------------------------------------------------------------------------------------------------
def test_clean_up_of_the_constructed_fixture(ctx):
    sv, sf, _ = gpu_mesh(ctx, 5, 20000)
    V, F, expect = mr.cleanup_fixture(sv, sf)
    nf = len(sf)
    assert expect == dict(removed_isolated=23792, removed_duplicate=3, removed_zero_area=2, removed_nonmanifold=3) and nf == 23792
    v, f, st = ctx.mesh_clean(V, F, smooth_steps=0)
    ev, ef, est = mr.clean(V, F, smooth_steps=0)
    assert np.array_equal(f, ef) and v.tobytes() == ev.tobytes()
    assert st == est
    assert {k: st[k] for k in expect} == expect and all(st[k] > 0 for k in expect)
    assert st["components"] == 4 and st["components_removed"] == 1 and st["n_faces"] == 2 * nf - 2 and st["vertices_dropped"] == len(sv) + 4
    # the 20 % copy stays: its vertices are the tail of the result, bit for bit
    assert v[-len(sv):].tobytes() == V[2 * len(sv):3 * len(sv)].tobytes()
    # each switch, turned off, leaves its faces in
    for kw in (dict(duplicates=False), dict(zero_area=False), dict(nonmanifold=False), dict(duplicates=False, nonmanifold=False),
               dict(duplicates=False, zero_area=False, nonmanifold=False), dict(min_piece=0.0)):
        v2, f2, s2 = ctx.mesh_clean(V, F, smooth_steps=0, **kw)
        e2v, e2f, e2s = mr.clean(V, F, smooth_steps=0, **kw)
        assert np.array_equal(f2, e2f) and v2.tobytes() == e2v.tobytes() and s2 == e2s, kw
    assert ctx.mesh_clean(V, F, smooth_steps=0, zero_area=False)[2]["n_faces"] == st["n_faces"] + 2
    assert ctx.mesh_clean(V, F, smooth_steps=0, nonmanifold=False)[2]["n_faces"] == st["n_faces"] + 3
    s = ctx.mesh_clean(V, F, smooth_steps=0, duplicates=False, nonmanifold=False)[2]
    assert s["removed_duplicate"] == 0 and s["n_faces"] == st["n_faces"] + 6
    # smoothing first, then the clean-up on the smoothed mesh
    v5, f5, s5 = ctx.mesh_clean(V, F)
    e5v, e5f, e5s = mr.clean(V, F)
    assert np.array_equal(f5, e5f) and v5.tobytes() == e5v.tobytes() and s5 == e5s


# ---- 4: thresholds and edge cases ---------------------------------------------------------------------------------------------------------
def test_thresholds_are_strict_and_exact(ctx):
    sv, sf, _ = gpu_mesh(ctx, 5, 20000)
    # one component, relative 1.0: its diameter equals D, and the comparison is strict
    v, f, st = ctx.mesh_clean(sv, sf, smooth_steps=0, min_piece=1.0, relative=True)
    assert st["components"] == 1 and st["components_removed"] == 0 and np.array_equal(f, sf) and v.tobytes() == sv.tobytes()
    assert st["threshold"] == st["diameter"] == float(mr.box_diameter(sv.min(0), sv.max(0))[0])
    # two pieces: an absolute threshold just above / just below the small one's fp64 diameter
    small = ((sv - sv.mean(0)) * np.float32(0.25) + np.float32([300.0, 0.0, 0.0])).astype(np.float32)
    V, F = np.concatenate([sv, small]), np.concatenate([sf, sf + len(sv)])
    d = float(mr.box_diameter(small.min(0), small.max(0))[0])
    for thr, gone in ((np.nextafter(d, np.inf), True), (d, False), (np.nextafter(d, 0.0), False)):
        v, f, st = ctx.mesh_clean(V, F, smooth_steps=0, min_piece=thr, relative=False)
        assert st["threshold"] == thr and st["components"] == 2 and st["components_removed"] == int(gone)
        assert st["removed_isolated"] == (len(sf) if gone else 0)
        assert st == mr.clean(V, F, smooth_steps=0, min_piece=thr, relative=False)[2]
    # min_piece = 0 removes nothing
    v, f, st = ctx.mesh_clean(V, F, smooth_steps=0, min_piece=0.0)
    assert st["removed_isolated"] == 0 and st["threshold"] == 0.0 and len(f) + st["removed_zero_area"] == len(F)


def test_empty_in_and_empty_out(ctx):
    e = np.zeros((0, 3))
    v, f, st = ctx.mesh_clean(e, e)
    assert v.shape == (0, 3) and f.shape == (0, 3) and st == mr.clean(e, e)[2] and st["n_vertices_in"] == 0
    sv, sf, _ = gpu_mesh(ctx, 5, 20000)
    v, f, st = ctx.mesh_clean(sv, e)                                                    # vertices without faces: all unused
    assert v.shape == (0, 3) and f.shape == (0, 3) and st == mr.clean(sv, e)[2] and st["vertices_dropped"] == len(sv)
    assert ctx.mesh_smooth(sv, e, 3).tobytes() == sv.tobytes()
    lab, n = ctx.mesh_components(e, 10)
    assert lab.shape == (0,) and n == 0
    # everything removed: an empty mesh, status 0
    v, f, st = ctx.mesh_clean(sv, sf, smooth_steps=1, min_piece=1e6, relative=False)
    assert v.shape == (0, 3) and f.shape == (0, 3) and st["removed_isolated"] == len(sf) and st["vertices_dropped"] == len(sv)
    assert st == mr.clean(sv, sf, smooth_steps=1, min_piece=1e6, relative=False)[2]
    assert ctx.poisson_last_mesh(0, 0)[0].shape == (0, 3)


def test_invalid_input_is_refused_and_named(ctx):
    from reconstruction_amd._lib import RSM_E_INVALID, MeshCleanParams
    lib, h = ctx._lib, ctx._h
    v, f = mr.grid_mesh(5, 5)
    nv, nf = C.c_int64(), C.c_int64()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(V=v, F=f, n_v=None, n_f=None, pn=C.byref(nv), **kw):
        p = MeshCleanParams(5, 1, 1, 0.1, 1, 7)
        for k, val in kw.items():
            setattr(p, k, val)
        st = lib.rsm_mesh_clean(h, ptr(V), C.c_int64(len(V) if n_v is None else n_v), ptr(F), C.c_int64(len(F) if n_f is None else n_f), C.byref(p), pn,
                                C.byref(nf), None)
        return st, (lib.rsm_last_error(h) or b"").decode()
    bad_i, neg_i, bad_c, inf_c = f.copy(), f.copy(), v.copy(), v.copy()
    bad_i[7, 1] = len(v)
    neg_i[0, 0] = -1
    bad_c[3, 2] = np.nan
    inf_c[24, 0] = np.inf
    for kw, name in ((dict(F=bad_i), "index"), (dict(F=neg_i), "index"), (dict(V=bad_c), "finite"), (dict(V=inf_c), "finite"),
                     (dict(n_f=(2 ** 31 + 2) // 3), "nf"), (dict(n_f=-1), "nf"), (dict(n_v=-1), "nv"), (dict(n_v=2 ** 31), "nv"),
                     (dict(smooth_steps=-1), "smooth_steps"), (dict(cotangent=2), "cotangent"), (dict(boundary=-1), "boundary"),
                     (dict(min_piece=-0.5), "min_piece"), (dict(min_piece=float("nan")), "min_piece"), (dict(min_piece=float("inf")), "min_piece"),
                     (dict(min_piece_relative=3), "min_piece_relative"), (dict(flags=8), "flags"), (dict(V=None, n_v=len(v)), "NULL"), (dict(F=None, n_f=len(f)), "NULL"),
                     (dict(pn=None), "NULL")):
        st, msg = call(**kw)
        assert st == RSM_E_INVALID and name in msg, (kw, st, msg)
    assert lib.rsm_mesh_clean(h, ptr(v), C.c_int64(len(v)), ptr(f), C.c_int64(len(f)), None, C.byref(nv), C.byref(nf), None) == RSM_E_INVALID
    assert "params" in (lib.rsm_last_error(h) or b"").decode()
    assert call()[0] == 0 and nf.value == len(f)
    # the stage entry points check the same inputs
    from reconstruction_amd import RsmError
    for fn in (lambda: ctx.mesh_smooth(v, bad_i, 1), lambda: ctx.mesh_smooth(bad_c, f, 1), lambda: ctx.mesh_components(bad_i, len(v)),
               lambda: ctx.mesh_smooth(v, f, -1), lambda: ctx.mesh_clean(v, neg_i)):
        with pytest.raises(RsmError) as e:
            fn()
        assert e.value.code == RSM_E_INVALID


def test_two_calls_and_all_three_entries_return_the_same_bytes(ctx):
    v0, f0, _ = gpu_mesh(ctx, 6, 80000, cap=True, trim=2)
    v1, f1, s1 = ctx.mesh_clean(v0, f0)
    v2, f2, s2 = ctx.mesh_clean(v0, f0)
    assert v1.tobytes() == v2.tobytes() and f1.tobytes() == f2.tobytes() and s1 == s2 and len(f1) > 1000
    # poisson_last_mesh afterwards returns the cleaned mesh
    hv, hf = ctx.poisson_last_mesh(len(v1), len(f1))
    assert hv.tobytes() == v1.tobytes() and hf.tobytes() == f1.tobytes()
    # device buffers
    dv, df = torch.from_numpy(v0).cuda(), torch.from_numpy(f0).cuda()
    nv, nf, s3 = ctx.mesh_clean_device(dv.data_ptr(), len(v0), df.data_ptr(), len(f0))
    assert (nv, nf) == (len(v1), len(f1)) and s3 == s1
    ov = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    of = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    ctx.poisson_last_mesh_device(ov.data_ptr(), of.data_ptr())
    torch.cuda.synchronize()
    assert ov.cpu().numpy().tobytes() == v1.tobytes() and of.cpu().numpy().tobytes() == f1.tobytes()
    # mesh_clean_last: the mesh the Poisson call left, cleaned where it lies, equals mesh_clean of the copied-out mesh
    xyz, nrm = pr.sphere_samples(80000, cap=True)
    pv, pf, _ = ctx.poisson_mesh(xyz, nrm, 6, trim_cells=2)
    assert pv.tobytes() == v0.tobytes() and pf.tobytes() == f0.tobytes()
    lv, lf, ls = ctx.mesh_clean_last()
    assert lv.tobytes() == v1.tobytes() and lf.tobytes() == f1.tobytes() and ls == s1
    hv, hf = ctx.poisson_last_mesh(len(v1), len(f1))
    assert hv.tobytes() == v1.tobytes() and hf.tobytes() == f1.tobytes()
    # and once more on its own result: the last mesh is the input again
    lv2, lf2, ls2 = ctx.mesh_clean_last(smooth_steps=0)
    e2v, e2f, e2s = mr.clean(v1, f1, smooth_steps=0)
    assert lv2.tobytes() == e2v.tobytes() and np.array_equal(lf2, e2f) and ls2 == e2s


# ---- 5: end to end ------------------------------------------------------------------------------------------------------------------------
def test_cloud_optimization_run_mesh_then_clean_mesh(ctx):
    from reconstruction_amd import Camera, CloudOptimization, ManageData, StereoMatching
    cfgs = [synth.config_small(320, 192, 3, radius=2, pair=4, mask_l0_width=60, border_l0=4),
            synth.config_small(320, 192, 3, radius=2, pair=5, mask_l0_width=50, border_l0=4, holes=True)]
    cam = np.array([0.0, 0.0, 0.0], np.float32)
    top = 1 << (cfgs[0].pyr_levels - 1)
    data = ManageData(cam=[[Camera(camID=0, image=c.image[0], mask=c.mask[0], CamCenter=cam),
                            Camera(camID=1, image=c.image[1], mask=c.mask[1], CamCenter=cam)] for c in cfgs],
                      m_PyrmNum=cfgs[0].pyr_levels, m_LowestLevelSize=(cfgs[0].width // top, cfgs[0].height // top),
                      m_OriginSize=(cfgs[0].width, cfgs[0].height),
                      rectified=[dict(Q=c.Q, R_final=c.R_final, T_final=c.T_final) for c in cfgs])
    opt = CloudOptimization(ctx)
    opt.Init(100, 1, 50, 2, 40.0, data, False)
    sm = StereoMatching(0)
    sm.Init(data, opt, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    opt.run()
    with pytest.raises(ValueError, match="mesh"):
        opt.clean_mesh()
    mv, mf, _ = opt.mesh(depth=7, trim_cells=4)
    v, f, st = opt.clean_mesh()
    assert opt.mesh_result[0] is v and opt.mesh_result[2] is st
    ev, ef, est = mr.clean(mv, mf)
    print("run() -> mesh() -> clean_mesh(): %d faces -> %d; %s" % (len(mf), len(f), st))
    assert np.array_equal(f, ef) and v.tobytes() == ev.tobytes() and st == est
    assert 0 < len(f) <= len(mf) and np.isfinite(v).all()
    rep = pr.manifold_report(v, f)
    assert rep["index_out_of_range"] == 0 and rep["repeated_index"] == 0 and rep["unused_vertices"] == 0


def test_cli_mesh_clean_writes_the_cleaned_bigmesh(ctx, tmp_path, capsys):
    from PIL import Image
    from reconstruction_amd import config as cfgmod
    from reconstruction_amd.__main__ import main
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
    norm = lambda s: re.sub(r"\d+\.\d+ s", "T s", s)
    base = [root + "config.yml", "--mls-radius", "10", "--mesh-depth", "7"]
    capsys.readouterr()
    assert main(base + ["--mesh", "--mesh-out", root + "raw.ply"]) == 0
    plain = norm(capsys.readouterr().out)
    assert "Mesh clean" not in plain
    rv, rf = pr.read_ply_mesh(root + "raw.ply")
    assert main(base + ["--mesh-clean"]) == 0                                            # implies --mesh
    out = norm(capsys.readouterr().out)
    v, f = pr.read_ply_mesh(root + "bigmesh.ply")
    ev, ef, est = mr.clean(rv, rf)
    assert np.array_equal(f, ef) and v.tobytes() == ev.tobytes()
    lines = out.splitlines()
    assert lines[:-2] == plain.splitlines()[:-1] and lines[-2].startswith("Mesh clean: %d of %d pieces removed" % (est["components_removed"], est["components"]))
    assert lines[-1] == "%d vertices, %d faces -> %sbigmesh.ply" % (len(v), len(f), root)
    # the options: no smoothing and an absolute length
    assert main(base + ["--mesh-clean", "--mesh-smooth", "0", "--mesh-min-piece", "25.5", "--mesh-out", root + "m2.ply"]) == 0
    v2, f2 = pr.read_ply_mesh(root + "m2.ply")
    e2v, e2f, _ = mr.clean(rv, rf, smooth_steps=0, min_piece=25.5, relative=False)
    assert np.array_equal(f2, e2f) and v2.tobytes() == e2v.tobytes()
    capsys.readouterr()
    assert main(base + ["--mesh-clean", "--mesh-smooth", "-2"]) == 1
    assert "smooth_steps" in capsys.readouterr().out


# ---- 6: the effect ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,n", [(5, 20000), (6, 80000)])
def test_five_cotangent_steps_lower_the_radial_error(ctx, depth, n):
    v, f, h = gpu_mesh(ctx, depth, n)
    p = ctx.mesh_smooth(v, f, 5, True, True)
    q = mr.smooth(v, f, 5, True, True)
    b, a, r = pr.radial_error_h(v, h), pr.radial_error_h(p, h), pr.radial_error_h(q, h)
    print("depth %d: radial error max %.4f h -> GPU %.4f h (restatement %.4f h), mean %.4f h -> GPU %.4f h (restatement %.4f h)"
          % (depth, b.max(), a.max(), r.max(), b.mean(), a.mean(), r.mean()))
    assert np.isfinite(p).all() and a.max() < b.max() and a.mean() < b.mean()
