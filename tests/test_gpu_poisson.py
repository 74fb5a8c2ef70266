"""GPU dense-grid Poisson surface and trim (csrc/k_poisson.hip) against the numpy restatement
(tests/poisson_restatement.py): the exact conditions (closed oriented manifold, trim, extraction, right-hand side, reproducibility,
edge cases), the measured quantities (geometry, field) held to the restatement's own figures, and the whole path behind
CloudOptimization.run() and the CLI.

Figures (MI355X; restatement solved to 1e-10, GPU to the default rel_residual 4e-5; h = grid spacing; depth 5 / depth 6):
  sphere, max radial error      restatement 0.2892 h / 0.2721 h     GPU 0.2892 h / 0.2721 h (10 / 11 cycles)      bound: twice the restatement's
  cap, own-cell vertices        restatement 0.7125 h / 0.7664 h     GPU 0.7127 h / 0.7664 h                       bound: twice the restatement's
  field max|chi - chi_ref| / range(chi_ref)
                                restatement at 4e-5 against itself at 1e-10: 5.5e-5 / 3.4e-4                      GPU 8.6e-6 / 2.1e-5, bound: four times that gap
  right-hand side               max |b - b_ref| 1.9e-9; the largest err / bound over the nodes 0.993 .. 1.000 (nodes with a single contribution rounded by almost half a unit)
  extraction                    faces identical, vertices identical bits (0 coordinates differ)
  depth 7, default against the floor (2.1e-6): 0.2927 h both
(profiles/f9_gpu_poisson_tests.log)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import poisson_restatement as pr
from reconstruction_amd import synth
from reconstruction_amd.api import POISSON_REL_RESIDUAL

pytestmark = pytest.mark.gpu

CLOSED = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0, edge_without_opposite=0, edges_not_in_two_faces=0, euler=2,
              unused_vertices=0)
CASES = [(5, 20000), (6, 80000)]
_cache = {}


def ref(depth, n, cap=False):
    """the restatement on the sphere / cap inputs, solved to 1e-10 (cached per session)"""
    key = (depth, n, cap)
    if key not in _cache:
        xyz, nrm = pr.sphere_samples(n, cap=cap)
        R = pr.reconstruct(xyz, nrm, depth)
        R["xyz"], R["nrm"] = xyz, nrm
        _cache[key] = R
    return _cache[key]


def grid_of(R):
    return np.array([R["o"][0], R["o"][1], R["o"][2], R["h"]])


# ---- 1, 2 and the geometry figure ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,n", CASES)
def test_sphere_is_a_closed_oriented_manifold_near_the_sphere(ctx, depth, n):
    R = ref(depth, n)
    v, f, st = ctx.poisson_mesh(R["xyz"], R["nrm"], depth, trim_cells=0)
    assert st["converged"] and st["residual"] <= POISSON_REL_RESIDUAL and st["n_valid"] == n and st["n_invalid"] == 0
    assert st["origin"] == tuple(R["o"]) and st["h"] == R["h"] and st["N"] == 1 << depth
    assert pr.manifold_report(v, f) == CLOSED
    # one vertex per lattice edge: an edge's vertex lies on that edge alone, so equal keys would show as equal positions
    assert len(np.unique(v, axis=0)) == len(v)
    assert pr.face_orientation_min(v, f) > 0.0
    err, rerr = pr.radial_error_h(v, st["h"]), pr.radial_error_h(R["verts"], R["h"])
    print("depth %d: GPU %d vertices %d faces, %d cycles, residual %.2e; radial error max %.4f h (restatement %.4f h), mean %.4f h"
          % (depth, len(v), len(f), st["cycles"], st["residual"], err.max(), rerr.max(), err.mean()))
    assert err.max() <= 2.0 * rerr.max()


@pytest.mark.parametrize("depth,n", CASES)
def test_cap_geometry_where_the_cell_holds_a_sample(ctx, depth, n):
    R = ref(depth, n, cap=True)
    v, f, st = ctx.poisson_mesh(R["xyz"], R["nrm"], depth, trim_cells=0)
    N = 1 << depth

    def own_cell_max(verts):
        c = pr.vertex_cells(verts, R["o"], R["h"], N)
        own = R["occ"][c[:, 2], c[:, 1], c[:, 0]] != 0
        return pr.radial_error_h(verts[own], R["h"]).max(), int(own.sum())
    g, ng = own_cell_max(v)
    r, nr = own_cell_max(R["verts"])
    print("depth %d cap: own-cell vertices GPU %d max %.4f h, restatement %d max %.4f h" % (depth, ng, g, nr, r))
    assert ng > 1000 and g <= 2.0 * r


# ---- 3: the trim is exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,n", CASES)
def test_trim_keeps_exactly_the_faces_inside_numpys_dilation(ctx, depth, n):
    R = ref(depth, n, cap=True)
    v0, f0, st = ctx.poisson_mesh(R["xyz"], R["nrm"], depth, trim_cells=0)
    assert st["origin"] == tuple(R["o"]) and st["h"] == R["h"]
    for t in (1, 2, 4):
        v, f, s = ctx.poisson_mesh(R["xyz"], R["nrm"], depth, trim_cells=t)
        ev, ef = pr.trim(v0, f0, R["occ"], R["o"], R["h"], t)       # numpy's occupancy, numpy's dilation, the GPU's untrimmed mesh
        assert 0 < len(ef) < len(f0)
        assert np.array_equal(f, ef) and v.tobytes() == ev.tobytes()
        assert s["n_faces_untrimmed"] == len(f0) and s["n_vertices_untrimmed"] == len(v0)


# ---- 4: extraction equals the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [False, True])
@pytest.mark.parametrize("depth,n", CASES)
def test_extraction_equals_the_restatement(ctx, depth, n, cap):
    """Faces identical and in the same order; vertices within 1 float32 ulp.  (Both sides evaluate pa + t (pb - pa), t = (iso - chi_a) /
    (chi_b - chi_a), in float32 in the same order without fused multiply-adds, so the vertices are in fact the same bits; the count of
    differing coordinates is printed.)"""
    R = ref(depth, n, cap)
    v, f = ctx.iso_mesh(R["chi32"], R["iso"], grid_of(R), R["occ"], 0)
    assert np.array_equal(f, R["faces0"])
    assert v.shape == R["verts0"].shape
    ulp = np.spacing(np.abs(R["verts0"]))
    print("depth %d cap %d: %d vertices, %d faces, coordinates that differ: %d" % (depth, cap, len(v), len(f), int((v != R["verts0"]).sum())))
    assert (np.abs(v.astype(np.float64) - R["verts0"].astype(np.float64)) <= ulp).all()
    if cap:
        for t in (1, 4):
            tv, tf = ctx.iso_mesh(R["chi32"], R["iso"], grid_of(R), R["occ"], t)
            ev, ef = pr.trim(R["verts0"], R["faces0"], R["occ"], R["o"], R["h"], t)
            assert np.array_equal(tf, ef) and (np.abs(tv.astype(np.float64) - ev.astype(np.float64)) <= np.spacing(np.abs(ev))).all()


# ---- 5: right-hand side ----------------------------------------------------------------------------------------------------------------
def check_rhs(ctx, R, xyz, nrm, depth, scale, label):
    """The GPU's step 1 to 4 (ctx.poisson_rhs) against the restatement's (R: its o, h, occ, cnt, b): grid, counts and occ equal, b within
    pr.rhs_fixed_point_bound node by node (the derivation is there).  Returns the GPU's (grid, b, occ)."""
    grid, b, occ, counts = ctx.poisson_rhs(xyz, nrm, depth, scale)
    assert np.array_equal(grid, np.array([R["o"][0], R["o"][1], R["o"][2], R["h"]])) and counts == (len(xyz), 0)
    assert np.array_equal(occ, R["occ"])
    bound = pr.rhs_fixed_point_bound(R["cnt"], R["b"])
    err = np.abs(b - R["b"])
    print("%s: max |b - b_ref| %.3e, max bound %.3e, max err / bound %.3f" % (label, err.max(), bound.max(), (err / bound).max()))
    assert (err <= bound).all()
    return grid, b, occ


@pytest.mark.parametrize("cap", [False, True])
@pytest.mark.parametrize("depth,n", CASES)
def test_rhs_within_the_fixed_point_bound(ctx, depth, n, cap):
    R = ref(depth, n, cap)
    check_rhs(ctx, R, R["xyz"], R["nrm"], depth, 1.1, "depth %d cap %d" % (depth, cap))


# ---- the field -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,n", CASES)
def test_field_against_the_restatement(ctx, depth, n):
    R = ref(depth, n)
    rng_ = R["chi"].max() - R["chi"].min()
    coarse, res = pr.solve(R["b"], POISSON_REL_RESIDUAL)
    gap = np.abs(coarse - R["chi"]).max() / rng_
    chi, gres, cyc, status, hist = ctx.poisson_solve(R["b"])
    fig = np.abs(chi.astype(np.float64) - R["chi"]).max() / rng_
    print("depth %d: restatement at %.0e against 1e-10: gap %.3e; GPU (%d cycles, residual %.2e): %.3e" % (depth, POISSON_REL_RESIDUAL, gap, cyc, gres, fig))
    assert status == 0 and gres <= POISSON_REL_RESIDUAL
    # the residual the library reports is the one chi has
    true = np.linalg.norm(R["b"].astype(np.float32).astype(np.float64) - pr.apply_L(chi.astype(np.float64))) / np.linalg.norm(R["b"].astype(np.float32))
    assert abs(true - gres) <= 0.05 * POISSON_REL_RESIDUAL
    assert fig <= 4.0 * gap


# ---- 6: reproducible -------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_both_entries_return_the_same_bytes(ctx):
    R = ref(6, 80000, cap=True)
    xyz, nrm = R["xyz"], R["nrm"]
    g1, b1, o1, _ = ctx.poisson_rhs(xyz, nrm, 6)
    g2, b2, o2, _ = ctx.poisson_rhs(xyz, nrm, 6)
    assert b1.tobytes() == b2.tobytes() and o1.tobytes() == o2.tobytes()
    c1 = ctx.poisson_solve(b1)[0]
    c2 = ctx.poisson_solve(b1)[0]
    assert c1.tobytes() == c2.tobytes()
    v1, f1, s1 = ctx.poisson_mesh(xyz, nrm, 6, trim_cells=2)
    v2, f2, s2 = ctx.poisson_mesh(xyz, nrm, 6, trim_cells=2)
    assert v1.tobytes() == v2.tobytes() and f1.tobytes() == f2.tobytes() and s1 == s2 and len(f1) > 1000
    dx, dn = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
    nv, nf, s3 = ctx.poisson_mesh_device(dx.data_ptr(), dn.data_ptr(), len(xyz), 6, trim_cells=2)
    assert (nv, nf) == (len(v1), len(f1)) and s3 == s1
    dv = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    df = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    ctx.poisson_last_mesh_device(dv.data_ptr(), df.data_ptr())
    torch.cuda.synchronize()
    assert dv.cpu().numpy().tobytes() == v1.tobytes() and df.cpu().numpy().tobytes() == f1.tobytes()
    hv, hf = ctx.poisson_last_mesh(nv, nf)
    assert hv.tobytes() == v1.tobytes() and hf.tobytes() == f1.tobytes()


# ---- 7: edges --------------------------------------------------------------------------------------------------------------------------
def test_nothing_to_mesh_is_an_empty_mesh(ctx):
    bad_x = np.array([[np.nan, 0, 0], [1, 2, 3], [np.inf, 0, 0], [5, 5, 5], [1, 1, 1]], np.float32)
    bad_n = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0], [np.nan, 0, 0, 0], [0, np.inf, 0, 0]], np.float32)
    for xyz, nrm, valid in ((bad_x, bad_n, 0), (np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), 0),
                            (np.tile(np.float32([[3, 4, 5]]), (10, 1)), np.tile(np.float32([[0, 0, 1, 0]]), (10, 1)), 10)):
        v, f, st = ctx.poisson_mesh(xyz, nrm, 5)
        assert v.shape == (0, 3) and f.shape == (0, 3) and st["status"] == 0
        assert st["n_valid"] == valid and st["n_invalid"] == len(xyz) - valid
    grid, b, occ, counts = ctx.poisson_rhs(np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), 5)   # the stage entry without samples
    assert not grid.any() and b.shape == (32, 32, 32) and not b.any() and not occ.any() and counts == (0, 0)


def test_invalid_samples_take_no_part(ctx):
    R = ref(5, 20000)
    bad_x = np.array([[np.nan, 0, 0], [1, 2, 3], [np.inf, 0, 0], [5, 5, 5]], np.float32)
    bad_n = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0], [np.nan, 0, 0, 0]], np.float32)
    v, f, st = ctx.poisson_mesh(R["xyz"], R["nrm"], 5, trim_cells=2)
    mx, mn = np.concatenate([bad_x[:2], R["xyz"], bad_x[2:]]), np.concatenate([bad_n[:2], R["nrm"], bad_n[2:]])
    v2, f2, st2 = ctx.poisson_mesh(mx, mn, 5, trim_cells=2)
    assert v2.tobytes() == v.tobytes() and f2.tobytes() == f.tobytes()
    assert st2["n_invalid"] == 4 and st2["n_valid"] == st["n_valid"] == 20000
    # normals of any length count by their direction
    v3, f3, _ = ctx.poisson_mesh(R["xyz"], np.concatenate([R["nrm"][:, :3] * 4.0, R["nrm"][:, 3:]], 1), 5, trim_cells=2)
    assert f3.tobytes() == f.tobytes() and v3.tobytes() == v.tobytes()


def test_invalid_parameters_are_named(ctx):
    from reconstruction_amd._lib import RSM_E_INVALID, PoissonParams
    lib, h = ctx._lib, ctx._h
    xyz, nrm = pr.sphere_samples(100)
    nv, nf = C.c_int64(), C.c_int64()

    def call(n=100, x=xyz, m=nrm, pv=C.byref(nv), device=False, **kw):
        p = PoissonParams(5, 1.1, 1e-5, 50, 4)
        for k, val in kw.items():
            setattr(p, k, val)
        fn = lib.rsm_poisson_mesh_device if device else lib.rsm_poisson_mesh
        st = fn(h, None if x is None else x.ctypes.data_as(C.c_void_p), None if m is None else m.ctypes.data_as(C.c_void_p), C.c_int64(n),
                C.byref(p), pv, C.byref(nf), None)
        return st, (lib.rsm_last_error(h) or b"").decode()
    for device in (False, True):
        for kw, name in ((dict(depth=4), "depth"), (dict(depth=10), "depth"), (dict(scale=0.99), "scale"), (dict(scale=float("nan")), "scale"),
                         (dict(scale=float("inf")), "scale"), (dict(rel_residual=0.0), "rel_residual"), (dict(rel_residual=1.0), "rel_residual"),
                         (dict(rel_residual=float("nan")), "rel_residual"), (dict(max_cycles=0), "max_cycles"), (dict(trim_cells=-1), "trim_cells"),
                         (dict(n=-1), "n "), (dict(n=2 ** 31), "n "), (dict(x=None), "NULL"), (dict(m=None), "NULL"), (dict(pv=None), "NULL")):
            st, msg = call(device=device, **kw)
            assert st == RSM_E_INVALID and name in msg, (kw, st, msg)
    assert lib.rsm_poisson_mesh(h, xyz.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p), C.c_int64(100), None, C.byref(nv), C.byref(nf),
                                None) == RSM_E_INVALID
    assert "params" in (lib.rsm_last_error(h) or b"").decode()
    assert call()[0] == 0


def test_max_cycles_reached_is_a_status_of_its_own(ctx):
    from reconstruction_amd._lib import RSM_W_NOT_CONVERGED
    R = ref(6, 80000)
    v, f, st = ctx.poisson_mesh(R["xyz"], R["nrm"], 6, trim_cells=0, max_cycles=1)
    assert st["status"] == RSM_W_NOT_CONVERGED == 1 and not st["converged"] and st["cycles"] == 1 and st["residual"] > POISSON_REL_RESIDUAL
    rep = pr.manifold_report(v, f)
    print("one cycle: residual %.3e, %d vertices, %d faces, %s" % (st["residual"], len(v), len(f), rep))
    assert len(f) > 1000 and rep["index_out_of_range"] == 0 and rep["repeated_index"] == 0 and rep["edges_not_in_two_faces"] == 0
    assert "cycles" in (ctx._lib.rsm_last_error(ctx._h) or b"").decode()


# ---- the default rel_residual --------------------------------------------------------------------------------------------------------
def test_default_residual_leaves_the_geometry_where_the_floor_has_it(ctx):
    """The sphere's geometry figure at depth 7 between the default rel_residual and the float32 solver's floor (a target it cannot
    reach: all cycles run): within 0.01 h."""
    xyz, nrm = pr.sphere_samples(320000)
    v, f, st = ctx.poisson_mesh(xyz, nrm, 7, trim_cells=0)
    vf, ff, sf = ctx.poisson_mesh(xyz, nrm, 7, trim_cells=0, rel_residual=1e-12, max_cycles=40)
    a, b = pr.radial_error_h(v, st["h"]).max(), pr.radial_error_h(vf, sf["h"]).max()
    print("depth 7: default %.0e -> residual %.2e in %d cycles, radial max %.4f h; floor residual %.2e after %d cycles, radial max %.4f h"
          % (POISSON_REL_RESIDUAL, st["residual"], st["cycles"], a, sf["residual"], sf["cycles"], b))
    assert st["converged"] and sf["residual"] < st["residual"]
    assert abs(a - b) <= 0.01


# ---- 9: the whole path ---------------------------------------------------------------------------------------------------------------
def check_mesh_file(path, min_faces):
    v, f = pr.read_ply_mesh(path)
    assert len(f) >= min_faces and np.isfinite(v).all()
    rep = pr.manifold_report(v, f)
    assert rep["index_out_of_range"] == 0 and rep["repeated_index"] == 0
    return v, f


def test_cloud_optimization_run_then_mesh(ctx, tmp_path):
    from reconstruction_amd import Camera, CloudOptimization, ManageData, StereoMatching, write_ply_mesh
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
    with pytest.raises(ValueError, match="run"):
        opt.mesh()
    sm = StereoMatching(0)
    sm.Init(data, opt, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    before = [a.copy() for a in opt.run()]
    v, f, st = opt.mesh(depth=7, trim_cells=4)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, opt.cloud_ms_normals))     # run()'s result is untouched
    assert st["n_valid"] + st["n_invalid"] == len(before[0]) and st["n_valid"] > 10000 and st["status"] in (0, 1)
    path = str(tmp_path / "bigmesh.ply")
    write_ply_mesh(path, v, f)
    rv, rf = check_mesh_file(path, 1000)
    assert rv.tobytes() == v.tobytes() and np.array_equal(rf, f)


def test_cli_mesh_writes_bigmesh_and_leaves_the_rest_alone(ctx, tmp_path, capsys):
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
    import os
    norm = lambda s: re.sub(r"\d+\.\d+ s", "T s", s)
    capsys.readouterr()
    assert main([root + "config.yml", "--mls", "--mls-radius", "10"]) == 0
    plain = norm(capsys.readouterr().out)
    assert not os.path.exists(root + "bigmesh.ply") and "Mesh" not in plain and "faces" not in plain
    kinds = [k for l in plain.splitlines() for k in ("Matching time", "points -> ", "MLS time") if k in l]
    assert kinds == ["Matching time", "points -> ", "MLS time", "points -> "]       # what the CLI printed before --mesh existed
    cloud = open(root + "bigcloud.ply", "rb").read()
    assert main([root + "config.yml", "--mesh", "--mls-radius", "10", "--mesh-depth", "7"]) == 0      # --mesh implies --mls
    meshed = norm(capsys.readouterr().out)
    assert meshed.startswith(plain) and len(meshed.splitlines()) == len(plain.splitlines()) + 2
    assert open(root + "bigcloud.ply", "rb").read() == cloud
    v, f = check_mesh_file(root + "bigmesh.ply", 1000)
    assert ("%d vertices, %d faces -> %sbigmesh.ply" % (len(v), len(f), root)) in meshed
    assert main([root + "config.yml", "--mesh", "--mls-radius", "10", "--mesh-depth", "7", "--mesh-trim", "2", "--mesh-out", root + "m2.ply"]) == 0
    v2, f2 = check_mesh_file(root + "m2.ply", 500)
    assert len(f2) < len(f)
    assert main([root + "config.yml", "--mesh", "--mls-radius", "10", "--mesh-depth", "12"]) == 1
    assert "depth" in capsys.readouterr().out
