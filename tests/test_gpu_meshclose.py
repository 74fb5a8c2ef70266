"""GPU hole closing (csrc/k_meshclose.hip) against the numpy restatement (tests/meshclose_restatement.py): labels, sizes,
W(0, L-1) and faces are the restatement's exactly -- the same faces in the same order, the same bits.  Integers apart, everything is fp64
+ - * sqrt in a fixed order and "the least c_k, the lowest k among equals", which no order of evaluation changes.  If bits differ, look for a
contracted multiply-add or another order of (W + W) + A; the comparison is not to be loosened."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import meshclose_restatement as mc
import poisson_restatement as pr
from reconstruction_amd import synth

pytestmark = pytest.mark.gpu


def bits(x):
    return np.float64(x).view(np.uint64)


def same_as_restatement(ctx, v, f, max_hole_size):
    """the whole call on a host mesh; returns (faces, stats, the restatement's info)"""
    wv, wf, wst, info = mc.close_holes(v, f, max_hole_size)
    ov, of, st = ctx.mesh_close_holes(v, f, max_hole_size)
    assert ov.tobytes() == np.ascontiguousarray(v, np.float32).tobytes() == wv.tobytes()
    assert of.dtype == np.int32 and of.shape == wf.shape and of.tobytes() == wf.tobytes()
    assert st == wst
    return of, st, info


# ---- 1: loops ---------------------------------------------------------------------------------------------------------------------------------
def loop_scenes():
    pv, pf = mc.plane(5, 5)
    bow = mc.remove_faces(pf, [1 * 4 + 1, 16 + 1 * 4 + 1, 2 * 4 + 2, 16 + 2 * 4 + 2])
    v, f = mc.cut_plane()
    return {"cut_plane": (len(v), f), "bow_tie": (len(pv), bow), "lone_triangle": (3, np.int32([[0, 1, 2]])), "against": (4, np.int32([[0, 1, 2], [0, 1, 3]])),
            "alike": (4, np.int32([[0, 1, 2], [1, 0, 3]])), "tetrahedron": (4, mc.TETRA_F), "repeated_index": (5, np.int32([[0, 1, 1], [2, 3, 4], [4, 4, 4]]))}


@pytest.mark.parametrize("name", ["cut_plane", "bow_tie", "lone_triangle", "against", "alike", "tetrahedron", "repeated_index"])
def test_border_labels_and_sizes_are_the_restatements(ctx, name):
    nv, f = loop_scenes()[name]
    want = mc.border_loops(f, nv)
    label, size, nc = ctx.mesh_border_loops(f, nv)
    print("%s: %d border entries in %d components, loops %s, open %s" % (name, want["n_border"], nc, sorted(len(r) for r in want["loops"].values()), want["open"]))
    assert np.array_equal(label, want["label"]) and np.array_equal(size, want["size"]) and nc == len(want["components"])
    if name == "cut_plane":
        assert sorted(set(size[size > 0].tolist())) == [3, 4, 6, 32] and (size[label == 0] == 32).all() and nc == 4
    if name == "bow_tie":
        assert nc == 3 and sorted(np.bincount(label[size == 0]).tolist())[-2:] == [4, 4]
    if name == "lone_triangle":
        assert label.tolist() == [0, 0, 0] and size.tolist() == [3, 3, 3]
    if name == "against":
        assert label.tolist() == [-1, 1, 1, -1, 4, 4] and size.tolist() == [-1, 0, 0, -1, 0, 0]
    if name == "tetrahedron":
        assert nc == 0 and (label == -1).all() and (size == -1).all()


# ---- 2: the fill's bytes ----------------------------------------------------------------------------------------------------------------------
def test_cut_plane_is_closed_to_the_restatements_bytes_twice_and_counts_add_up(ctx):
    v, f = mc.cut_plane()
    of, st, info = same_as_restatement(ctx, v, f, 30)
    print("cut plane: %s" % st)
    assert (st["loops"], st["loops_closed"], st["loops_too_long"], st["faces_added"], st["longest_closed"], st["longest_loop"]) == (4, 3, 1, 7, 6, 32)
    assert mc.check_closed(v, f, of, info) == 13                                    # independent of the restatement's tables
    of2 = same_as_restatement(ctx, v, f, 30)[0]
    assert of2.tobytes() == of.tobytes()
    # the result is the context's last mesh; what is closed stays closed
    hv, hf = ctx.poisson_last_mesh(len(v), len(of))
    assert hv.tobytes() == v.tobytes() and hf.tobytes() == of.tobytes()
    _, of3, st3 = ctx.mesh_close_holes_last(30)
    assert of3.tobytes() == of.tobytes() and (st3["loops"], st3["faces_added"], st3["border_entries"]) == (1, 0, 32)
    # the device entry, and the outer border at 32
    dv, df = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    nv, nf, st4 = ctx.mesh_close_holes_device(dv.data_ptr(), len(v), df.data_ptr(), len(f), 32)
    wf = mc.close_holes(v, f, 32)[1]
    out = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    ctx.poisson_last_mesh_device(0, out.data_ptr())
    torch.cuda.synchronize()
    assert nv == len(v) and out.cpu().numpy().tobytes() == wf.tobytes() and st4["loops_closed"] == 4 and st4["longest_closed"] == 32


# ---- 3: thresholds ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,max_hole", [(30, 30), (31, 30), (64, 64), (65, 64), (16, 64), (17, 64), (33, 64)])
def test_annulus_closes_up_to_the_threshold(ctx, L, max_hole):
    """the inner border (L) closes up to the threshold and the outer one (2 L) stays open beside it; at 16 and 17 both close, in one call
    whose table is sized by the longer"""
    v, f = mc.annulus(L)
    of, st, info = same_as_restatement(ctx, v, f, max_hole)
    print("annulus %d at %d: %s" % (L, max_hole, st))
    closed = [n for n in (L, 2 * L) if n <= max_hole]
    assert len(closed) == {(30, 30): 1, (31, 30): 0, (64, 64): 1, (65, 64): 0, (16, 64): 2, (17, 64): 2, (33, 64): 1}[(L, max_hole)]
    assert (st["loops"], st["loops_closed"], st["loops_too_long"], st["longest_loop"]) == (2, len(closed), 2 - len(closed), 2 * L)
    assert len(of) == len(f) + sum(n - 2 for n in closed) and st["longest_closed"] == max(closed, default=0)
    mc.check_closed(v, f, of, info)


@pytest.mark.parametrize("L", [3, 4, 5, 9, 16, 17, 32, 33, 63, 64])
def test_ring_triangulation_is_the_restatements_bits(ctx, L):
    for seed in (0, 1):
        p = mc.ring_points(L, seed)
        ww, wt = mc.triangulate(p)
        w, t = ctx.mesh_hole_triangulate(p)
        print("L %d seed %d: W %.17g (restatement %.17g), triangles differing %d" % (L, seed, w, ww, int((t != wt).any(1).sum()) if t.shape == wt.shape else -1))
        assert bits(w) == bits(ww) and t.shape == (L - 2, 3) and np.array_equal(t, wt)
        if L <= 9:
            best = mc.brute_force(p)[0]
            assert abs(w - best) <= 4 * L * np.spacing(best)
        if L >= 4:                                                               # a forbidden diagonal the free optimum uses
            i, k, j = next(x for x in wt.tolist() if max(x[1] - x[0], x[2] - x[1]) >= 2)
            F = np.zeros((L, L), bool)
            F[(i, k) if k - i >= 2 else (k, j)] = True
            ww2, wt2 = mc.triangulate(p, F)
            w2, t2 = ctx.mesh_hole_triangulate(p, F)
            assert bits(w2) == bits(ww2) and np.array_equal(t2, wt2) and w2 >= w
            if L <= 9:
                best2 = mc.brute_force(p, F)[0]
                assert (w2 == best2 == np.inf) if best2 == np.inf else abs(w2 - best2) <= 4 * L * np.spacing(best2)


# ---- 4: rules 6 - 7 -----------------------------------------------------------------------------------------------------------------------------
def test_forbidden_diagonal_collinear_points_and_rings_without_a_triangulation(ctx):
    # the tetrahedron with two faces off: the surviving edge is not used again
    f = np.int32([[1, 2, 0], [3, 1, 0]])
    of, st, _ = same_as_restatement(ctx, mc.TETRA_V, f, 30)
    assert of.tolist() == [[1, 2, 0], [3, 1, 0], [2, 3, 0], [2, 1, 3]]
    d = mc.directed_counts(of)
    assert len(d) == 12 and all(c == 1 and d[(b, a)] == 1 for (a, b), c in d.items())
    # ties go to the lowest k
    sq = np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    w, t = ctx.mesh_hole_triangulate(sq)
    assert w == 1.0 and t.tolist() == [[0, 1, 3], [1, 2, 3]]
    # three collinear points on the ring: the ear without area is not used
    ring = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]])
    w, t = ctx.mesh_hole_triangulate(ring)
    ww, wt = mc.triangulate(ring)
    P = mc._points(ring)
    assert w == ww == 4.0 and np.array_equal(t, wt) and all(mc.tri_n2(P[i], P[k], P[j]) > 0.0 for i, k, j in t.tolist())
    # no admissible triangulation: every diagonal forbidden, or three collinear points
    w, t = ctx.mesh_hole_triangulate(sq, np.ones((4, 4), bool))
    assert w == np.inf and t.shape == (0, 3)
    p9 = mc.ring_points(9, 2)
    F = np.ones((9, 9), bool)
    w, t = ctx.mesh_hole_triangulate(p9, F)
    assert w == np.inf and t.shape == (0, 3) and mc.triangulate(p9, F)[0] == np.inf
    w, t = ctx.mesh_hole_triangulate(ring[:3])
    assert w == np.inf and t.shape == (0, 3)
    # ... and in a mesh: left whole and counted
    v, f = mc.collinear_hole()
    of, st, _ = same_as_restatement(ctx, v, f, 8)
    assert np.array_equal(of, f) and (st["loops_untriangulated"], st["loops_closed"], st["loops_too_long"], st["faces_added"]) == (1, 0, 1, 0)
    # the bow-tie's holes are open; its outer border of 16 is closed
    pv, pf = mc.plane(5, 5)
    bow = mc.remove_faces(pf, [5, 16 + 5, 10, 16 + 10])
    of, st, _ = same_as_restatement(ctx, pv, bow, 30)
    assert (st["open_components"], st["loops_closed"], st["faces_added"]) == (2, 1, 14)


# ---- 5: many holes ------------------------------------------------------------------------------------------------------------------------------
def test_many_holes_cross_a_block_of_the_compaction_and_come_in_ascending_label(ctx):
    v, f, holes = mc.many_holes()
    of, st, info = same_as_restatement(ctx, v, f, 30)
    print("many holes: %s" % st)
    assert holes > 256 and st["loops_closed"] == holes and st["loops_too_long"] == 1 and st["longest_loop"] == 140
    assert list(info["closed"]) == sorted(info["closed"]) and mc.check_closed(v, f, of, info) == st["border_entries"] - 140


# ---- 6: refusals, the empty mesh, the colours ---------------------------------------------------------------------------------------------------
def test_invalid_input_is_refused_and_named(ctx):
    from reconstruction_amd import RsmError
    from reconstruction_amd._lib import RSM_E_INVALID, MeshCloseParams
    lib, h = ctx._lib, ctx._h
    v, f = mc.plane(5, 5)
    nv, nf = C.c_int64(), C.c_int64()
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(V=v, F=f, n_v=None, n_f=None, pn=C.byref(nv), m=30):
        p = MeshCloseParams(m)
        st = lib.rsm_mesh_close_holes(h, ptr(V), C.c_int64(len(V) if n_v is None else n_v), ptr(F), C.c_int64(len(F) if n_f is None else n_f), C.byref(p), pn,
                                      C.byref(nf), None)
        return st, (lib.rsm_last_error(h) or b"").decode()
    bad_i, neg_i, bad_c = f.copy(), f.copy(), v.copy()
    bad_i[7, 1] = len(v)
    neg_i[0, 0] = -1
    bad_c[3, 2] = np.nan
    for kw, name in ((dict(m=2), "max_hole_size"), (dict(m=65), "max_hole_size"), (dict(m=-1), "max_hole_size"), (dict(F=bad_i), "index"), (dict(F=neg_i), "index"),
                     (dict(V=bad_c), "finite"), (dict(n_f=(2 ** 31 + 2) // 3), "nf"), (dict(n_f=-1), "nf"), (dict(n_v=-1), "nv"), (dict(n_v=2 ** 31), "nv"),
                     (dict(V=None, n_v=len(v)), "NULL"), (dict(F=None, n_f=len(f)), "NULL"), (dict(pn=None), "NULL")):
        st, msg = call(**kw)
        assert st == RSM_E_INVALID and name in msg and msg.startswith("mesh_close_holes"), (kw, st, msg)
    assert lib.rsm_mesh_close_holes(h, ptr(v), C.c_int64(len(v)), ptr(f), C.c_int64(len(f)), None, C.byref(nv), C.byref(nf), None) == RSM_E_INVALID
    assert "params" in (lib.rsm_last_error(h) or b"").decode()
    assert lib.rsm_mesh_close_holes_last(h, None, C.byref(nv), C.byref(nf), None) == RSM_E_INVALID
    p = MeshCloseParams(30)
    assert lib.rsm_mesh_close_holes_last(h, C.byref(p), None, C.byref(nf), None) == RSM_E_INVALID
    assert lib.rsm_mesh_close_holes_device(h, None, C.c_int64(3), None, C.c_int64(1), C.byref(p), C.byref(nv), C.byref(nf), None) == RSM_E_INVALID
    assert call()[0] == 0 and call(m=3)[0] == 0 and call(m=64)[0] == 0
    for fn in (lambda: ctx.mesh_close_holes(v, f, 2), lambda: ctx.mesh_close_holes_last(65), lambda: ctx.mesh_border_loops(bad_i, len(v)),
               lambda: ctx.mesh_border_loops(neg_i, len(v)), lambda: ctx.mesh_hole_triangulate(v[:2]), lambda: ctx.mesh_hole_triangulate(np.zeros((65, 3), np.float32)),
               lambda: ctx.mesh_hole_triangulate(bad_c[:5])):
        with pytest.raises(RsmError) as e:
            fn()
        assert e.value.code == RSM_E_INVALID and "mesh_close_holes" in str(e.value)


def test_empty_meshes_a_context_without_a_mesh_and_the_colours(ctx):
    from reconstruction_amd import Context, RsmError
    from reconstruction_amd._lib import RSM_E_STATE
    v, f = mc.plane(5, 5)
    e3, e3i = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    ov, of, st = ctx.mesh_close_holes(e3, e3i)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and st == mc.close_holes(e3, e3i)[2]
    ov, of, st = ctx.mesh_close_holes(v, e3i)                                     # the vertices are untouched, faces or none
    assert ov.tobytes() == v.tobytes() and of.shape == (0, 3) and st == mc.close_holes(v, e3i)[2]
    lab, size, nc = ctx.mesh_border_loops(e3i, 7)
    assert lab.shape == (0,) and size.shape == (0,) and nc == 0
    # a fresh context has no mesh: as rsm_mesh_clean_last there, an empty mesh and RSM_OK
    fresh = Context(0)
    cv, cf, cst = fresh.mesh_clean_last()
    ov, of, st = fresh.mesh_close_holes_last()
    assert cv.shape == ov.shape == (0, 3) and cf.shape == of.shape == (0, 3) and st["n_faces"] == 0 and st["n_vertices_in"] == 0
    # the colours of the last mesh go with the mesh they belonged to
    cv_, cf_ = mc.cut_plane()
    P = np.array([[100.0, 0, 0, 0], [0, 100.0, 0, 0], [0, 0, 1.0, 20.0]])
    from reconstruction_amd import Camera
    img = np.full((64, 64, 3), 90, np.uint8)
    cams = [[Camera(camID=0, image=img, mask=None, P=P), Camera(camID=1, image=img, mask=None, P=P)]]
    ctx.mesh_close_holes(cv_, cf_, 3)
    rgb, best, kst = ctx.mesh_color_last(cams, 0.5)
    assert len(rgb) == len(cv_)
    rgb2 = np.zeros((len(cv_), 3), np.uint8)
    assert ctx._lib.rsm_mesh_last_colors(ctx._h, rgb2.ctypes.data_as(C.c_void_p), None) == 0
    ctx.mesh_close_holes_last(30)
    assert ctx._lib.rsm_mesh_last_colors(ctx._h, rgb2.ctypes.data_as(C.c_void_p), None) == RSM_E_STATE
    rgb3, _, _ = ctx.mesh_color_last(cams, 0.5)                                   # the closed mesh is coloured like any other
    assert len(rgb3) == len(cv_)


# ---- 7: API and CLI -------------------------------------------------------------------------------------------------------------------------------
def test_cloud_optimization_run_mesh_trim_clean_then_close(ctx):
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
    sx, sn, _ = opt.run()
    with pytest.raises(ValueError, match="mesh"):
        opt.close_mesh_holes()
    mv, mf, mst = opt.mesh(depth=7, trim_cells=0)
    t = float(np.median(ctx.mesh_density(sx, sn, mv, 7)[1]))
    opt.trim_mesh(smooth_steps=5, trim=t)
    cv, cf, cst = opt.clean_mesh()
    opt.mesh_colors = "stale"
    v, f, st = opt.close_mesh_holes()
    assert opt.mesh_result[0] is v and opt.mesh_result[2] is st and opt.mesh_colors is None
    wv, wf, wst, info = mc.close_holes(cv, cf, 30)
    print("run() -> mesh() -> trim_mesh() -> clean_mesh() -> close_mesh_holes(): %d faces -> %d; %s" % (len(cf), len(f), st))
    assert v.tobytes() == cv.tobytes() == wv.tobytes() and f.tobytes() == wf.tobytes() and st == wst
    mc.check_closed(cv, cf, f, info)
    v2, f2, st2 = opt.close_mesh_holes(max_hole_size=64)
    w2 = mc.close_holes(v, f, 64)
    assert f2.tobytes() == w2[1].tobytes() and st2 == w2[2]


def test_cli_mesh_close_holes(ctx, tmp_path, capsys):
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
    assert main(base + ["--mesh-clean", "--mesh-out", root + "clean.ply"]) == 0
    plain = norm(capsys.readouterr().out)
    assert "close holes" not in plain
    cv, cf = pr.read_ply_mesh(root + "clean.ply")
    assert main(base + ["--mesh-clean", "--mesh-close-holes", "40"]) == 0
    out = norm(capsys.readouterr().out)
    v, f = pr.read_ply_mesh(root + "bigmesh.ply")
    wv, wf, wst, _ = mc.close_holes(cv, cf, 40)
    assert v.tobytes() == wv.tobytes() and np.array_equal(f, wf)
    lines = out.splitlines()
    assert lines[:-2] == plain.splitlines()[:-1]
    assert lines[-2].startswith("Mesh close holes: %d of %d loops closed with %d faces" % (wst["loops_closed"], wst["loops"], wst["faces_added"]))
    assert lines[-1] == "%d vertices, %d faces -> %sbigmesh.ply" % (len(v), len(f), root)
    # given bare, N is script2.mlx's 30, and the flag implies --mesh
    assert main(base + ["--mesh-out", root + "m30.ply", "--mesh-close-holes"]) == 0
    o30 = capsys.readouterr().out
    assert main(base + ["--mesh", "--mesh-out", root + "m.ply"]) == 0
    capsys.readouterr()
    pv, pf = pr.read_ply_mesh(root + "m.ply")
    v30, f30 = pr.read_ply_mesh(root + "m30.ply")
    w30 = mc.close_holes(pv, pf, 30)
    assert v30.tobytes() == pv.tobytes() and np.array_equal(f30, w30[1])
    assert "Mesh close holes: %d of %d loops closed with %d faces" % (w30[2]["loops_closed"], w30[2]["loops"], w30[2]["faces_added"]) in o30
    assert main(base + ["--mesh-close-holes", "65"]) == 1
    assert "max_hole_size" in capsys.readouterr().out
