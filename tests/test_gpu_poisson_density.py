"""The density-adaptive form of the GPU Poisson surface (csrc/k_poisson_density.hip) against its numpy restatement
(tests/poisson_density_restatement.py, held to hand-worked answers without a GPU in tests/test_poisson_density_cpu.py): rho, w and the
right-hand side to the bit with the restatement's depths handed in, the depths themselves within f11's cap on log2, the weighted
iso-value, the whole path on the two thinned spheres, repeatability, the refusals, and the API / CLI switch.  Depths 5 and 6 only.

Figures (MI355X; profiles/f35_poisson_density_tests.log; 38 tests in 6.5 s):
  exact splat      rho, w and all N^3 doubles of b are the restatement's bits on every input (setup B; plate and torus at scale 1 with 50 samples per
                   node: every sample below depth 5, the least at 3; constructed depths at n = 255, 256, 257; rows that take no part mixed in)
  depths           max |d - restatement| 8.9e-16 over the sweep (cap 1e-12), b then still differs by nothing; weight sums equal in every digit
  iso              |GPU - restatement on the GPU's chi| 2.2e-19 (B), 0 (A, plate); bounds 2.3e-13, 1.7e-12, 3.8e-15; the unweighted mean of the
                   same chi differs in the second digit (-6.42e-4 against -6.57e-4 on B)
  whole path       A (depth 6): sparse side max 0.6540 h (rms 0.3257), dense side 0.3428 h, the restatement's in every printed digit; the plain
                   call 21.32 h / 0.3507 h; 92 564 faces, 12 cycles, 1 322 of 30 792 samples below depth 6, least 3.224
                   B (depth 5): 0.2656 h (rms 0.0728) / 0.2948 h; the plain call 8.78 h / 0.3698 h; 23 260 faces, 10 cycles, 1 805 of 32 905
  rig              run() -> mesh(depth=6, samples_per_node=2): 15 049 faces (plain 5 316), 80 of 55 303 samples below depth 6, least 4.913"""
import ctypes as C
import re

import numpy as np
import pytest

import poisson_density_restatement as pd
import poisson_restatement as pr
from reconstruction_amd import RsmError, _lib, synth

pytestmark = pytest.mark.gpu

CLOSED = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0, edge_without_opposite=0, edges_not_in_two_faces=0, unused_vertices=0, euler=2)
_cache = {}


def same_bits(a, b):
    """(a call, so that a failure shows False and not a diff of two long byte strings)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def random_cloud(n, seed):
    """n points in a box away from the origin with random unit normals"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform([-40.0, 10.0, 300.0], [24.0, 74.0, 364.0], size=(n, 3))
    d = rng.normal(size=(n, 3))
    return pr._with_normals(xyz, d / np.linalg.norm(d, axis=1)[:, None])


# (samples, depth, scale, samples_per_node): the plate and the torus are evenly sampled, and 50 per node spreads them over the levels 3..5
SETS = {"B": (lambda: pd.setup_samples("B"), 5, 1.1, 2.0), "A": (lambda: pd.setup_samples("A"), 6, 1.1, 2.0),
        "plate": (lambda: pr.plate_samples(6001), 5, 1.0, 50.0), "torus": (lambda: pr.torus_samples(9000), 5, 1.0, 50.0)}
BAD_X = np.array([[np.nan, 0, 0], [1, 2, 3], [np.inf, 0, 0], [5, 5, 5], [0, -np.inf, 1]], np.float32)
BAD_N = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0], [np.nan, 0, 0, 0], [1, 0, 0, 0]], np.float32)


def with_bad_rows(xyz, nrm):
    """rows that take no part at the front (2), in the middle (2) and at the end (1); the mask of the original rows"""
    m = len(xyz) // 2
    x = np.concatenate([BAD_X[:2], xyz[:m], BAD_X[2:4], xyz[m:], BAD_X[4:]])
    n = np.concatenate([BAD_N[:2], nrm[:m], BAD_N[2:4], nrm[m:], BAD_N[4:]])
    keep = np.ones(len(x), bool)
    keep[[0, 1, 2 + m, 3 + m, len(x) - 1]] = False
    return x, n, keep


def samples_of(name):
    return cached(("samples", name), SETS[name][0])


def ref_of(name, kd=0, spn=None):
    xyz, nrm = samples_of(name)
    spn = SETS[name][3] if spn is None else spn
    return cached(("ref", name, kd, spn), lambda: pd.rhs_of(xyz, nrm, SETS[name][1], SETS[name][2], kd, spn))


def check_exact(ctx, xyz, nrm, depth, scale, kd, spn, R, label):
    """with the restatement's d handed in: rho, w, d, b, occ, counts and grid are the restatement's bits"""
    ok = R["ok"]
    d_rows = pd.expand(R["d"], ok)
    grid, b, occ, counts, rho, w, d = ctx.poisson_rhs_weighted(xyz, nrm, depth, scale, spn, kd, depth_in=d_rows)
    nz = int(np.count_nonzero(b))
    print("%s: n %d (%d valid), kd %d, spn %g: %d samples below depth %d, least d %.4f, b has %d non-zero nodes, max |b| %.3e"
          % (label, len(xyz), ok.sum(), R["kd"], spn, (R["d"] < depth).sum(), depth, R["d"].min(), nz, np.abs(b).max()))
    assert counts == (int(ok.sum()), int((~ok).sum()))
    assert np.array_equal(grid, np.array([R["o"][0], R["o"][1], R["o"][2], R["h"]]))
    assert same_bits(rho, pd.expand(R["rho"], ok)) and same_bits(w, pd.expand(R["w"], ok)) and same_bits(d, d_rows)
    assert np.array_equal(occ, R["occ"])
    assert nz > 0 and same_bits(b, R["b"])
    return grid, b


def check_depths(ctx, xyz, nrm, depth, scale, kd, spn, R, label):
    """without depth_in: d within 1e-12 of the restatement's (two log2 implementations), rho and w still its bits"""
    ok = R["ok"]
    grid, b, occ, counts, rho, w, d = ctx.poisson_rhs_weighted(xyz, nrm, depth, scale, spn, kd)
    gap = np.abs(d[ok] - R["d"]).max()
    print("%s: max |d - restatement| %.3e; b: max |GPU - restatement| %.3e of max |b| %.3e" % (label, gap, np.abs(b - R["b"]).max(), np.abs(R["b"]).max()))
    assert same_bits(rho, pd.expand(R["rho"], ok)) and same_bits(w, pd.expand(R["w"], ok))
    assert gap <= 1e-12 and not d[~ok].any()
    return d


# ---- 1: the exact splat ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "plate", "torus"])
@pytest.mark.parametrize("bad", [False, True])
def test_rhs_is_the_restatements_bits(ctx, name, bad):
    """plate and torus at scale 1: samples on the box's faces, so coarse splats are clipped and the prolongation reads outside the grid"""
    xyz, nrm = samples_of(name)
    depth, scale, spn = SETS[name][1:]
    R = ref_of(name)
    if bad:
        xyz, nrm, keep = with_bad_rows(xyz, nrm)
        R = dict(R, ok=keep)                      # the valid samples, and so every figure of theirs, are the same
    assert (R["d"] < depth).sum() > 50 and len(xyz) % 256 != 0
    check_exact(ctx, xyz, nrm, depth, scale, 0, spn, R, "%s%s" % (name, " with rows that take no part" if bad else ""))


@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("bad", [False, True])
def test_rhs_with_constructed_depths(ctx, n, bad):
    """depth_in holds exact integers (fr = 0), 3.0, depth, values below 3 and above depth; the last block is full, one short, one over"""
    xyz, nrm = random_cloud(n, 40 + n)
    din = np.resize(np.array([3.0, 4.0, 5.0, 2.5, 0.0, 7.25, 3.5, 4.75, -1.0, 100.0, 4.0 - 2.0 ** -40, 3.0 + 2.0 ** -50]), n)
    if bad:
        xyz, nrm, keep = with_bad_rows(xyz, nrm)
        rows = np.zeros(len(xyz))
        rows[keep] = din
        din = rows
    R = pd.rhs_of(xyz, nrm, 5, 1.1, 0, 2.0, d=din)
    assert set(np.unique(R["d"])) >= {3.0, 4.0, 5.0, 3.5, 4.75} and R["d"].min() == 3.0 and R["d"].max() == 5.0
    for L in (3, 4, 5):
        assert R["V"][L].any()
    grid, b, occ, counts, rho, w, d = ctx.poisson_rhs_weighted(xyz, nrm, 5, 1.1, 2.0, 0, depth_in=din)
    ok = R["ok"]
    print("n %d%s: %d valid, levels' non-zero nodes %s, max |b| %.3e" % (n, " with rows that take no part" if bad else "", ok.sum(),
                                                                          [int(np.count_nonzero(R["V"][L])) for L in (3, 4, 5)], np.abs(b).max()))
    assert counts == (int(ok.sum()), int((~ok).sum())) and ok.sum() == n
    assert same_bits(d, pd.expand(R["d"], ok)) and same_bits(rho, pd.expand(R["rho"], ok)) and same_bits(w, pd.expand(R["w"], ok))
    assert np.array_equal(occ, R["occ"]) and same_bits(b, R["b"])


# ---- 2: the depths, and the parameters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kd", [("B", 3), ("B", 4), ("B", 5), ("A", 0)])
@pytest.mark.parametrize("spn", [0.5, 2.0, 3.0, 50.0])
def test_parameter_sweep(ctx, name, kd, spn):
    """kernel depths 3, 4, 5 at depth 5 and 0 (= 4) at depth 6; samples_per_node 50 drives many samples down to level 3"""
    xyz, nrm = samples_of(name)
    depth, scale = SETS[name][1:3]
    R = ref_of(name, kd, spn)
    label = "%s depth %d kd %d spn %g" % (name, depth, kd, spn)
    check_exact(ctx, xyz, nrm, depth, scale, kd, spn, R, label)
    d = check_depths(ctx, xyz, nrm, depth, scale, kd, spn, R, label)
    if spn == 50.0:
        assert (R["d"] == 3.0).sum() > 100
    st = ctx.poisson_mesh_weighted(xyz, nrm, depth, scale, trim_cells=0, samples_per_node=spn, kernel_depth=kd)[2]
    ok = R["ok"]
    print("%s: stats kernel_depth %d, min_sample_depth %.6f, n_below_depth %d, weight_sum %.17g (restatement %.17g)"
          % (label, st["kernel_depth"], st["min_sample_depth"], st["n_below_depth"], st["weight_sum"], R["w"].sum()))
    assert (st["n_valid"], st["n_invalid"]) == (int(ok.sum()), int((~ok).sum())) and st["kernel_depth"] == R["kd"]
    assert st["min_sample_depth"] == d[ok].min() and st["n_below_depth"] == int((d[ok] < depth).sum()) == int((R["d"] < depth).sum())
    assert abs(st["weight_sum"] - R["w"].sum()) <= len(R["w"]) * 2.0 ** -52 * R["w"].max()


# ---- 3: the iso-value ----------------------------------------------------------------------------------------------------------------------------
def stage_chain(ctx, name):
    def make():
        xyz, nrm = samples_of(name)
        depth, scale, spn = SETS[name][1:]
        grid, b, occ, counts, rho, w, d = ctx.poisson_rhs_weighted(xyz, nrm, depth, scale, spn, 0)
        chi = ctx.poisson_solve(b)[0]
        v, f, st = ctx.poisson_mesh_weighted(xyz, nrm, depth, scale, trim_cells=0, samples_per_node=spn)
        return grid, chi, w, v, f, st
    return cached(("chain", name), make)


@pytest.mark.parametrize("name", ["B", "A", "plate"])
def test_iso_value_is_the_weighted_mean_of_chi_at_the_valid_samples(ctx, name):
    """Both sides sum n fp64 terms w chi bounded by max w max|chi| in their own order and divide by sum w >= n min w: the means agree within
    n 2^-52 max|chi| (max w / min w)."""
    R = ref_of(name)
    grid, chi, w, v, f, st = stage_chain(ctx, name)
    n = len(R["p"])
    assert same_bits(w[R["ok"]], R["w"])
    iso = pd.iso_value(chi, R["p"], R["w"], R["o"], R["h"])
    plain = pr.iso_value(chi, R["p"], R["o"], R["h"])
    bound = n * 2.0 ** -52 * np.abs(chi).max() * (R["w"].max() / R["w"].min())
    print("%s: iso %.17g, restatement on the GPU's chi %.17g, difference %.3e, bound %.3e; the unweighted mean %.17g" % (name, st["iso"], iso, abs(st["iso"] - iso), bound, plain))
    assert st["n_valid"] == n and abs(st["iso"] - iso) <= bound and abs(plain - iso) > 100.0 * bound
    sv, sf = ctx.iso_mesh(chi, st["iso"], grid)
    assert len(f) > 1000 and same_bits(sv, v) and same_bits(sf, f)


# ---- 4: the whole path ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_thinned_sphere_holds_its_place(ctx, name):
    """The surface is closed and oriented, and its error figures are the restatement's within 0.01 h: ten times the largest gap between the
    GPU and the restatement that DESIGN.md 9 f7 records for such figures (0.289 vs 0.2892, 0.766 vs 0.7664).  The plain call caves in."""
    xyz, nrm = samples_of(name)
    depth, scale = SETS[name][1:3]
    R = cached(("whole", name), lambda: pd.reconstruct(xyz, nrm, depth, scale, 0, 2.0))
    v, f, st = ctx.poisson_mesh_weighted(xyz, nrm, depth, scale, trim_cells=0, samples_per_node=2.0)
    (gs, gs_rms), (gd, gd_rms) = pd.side_errors(v, st["h"])
    (rs, rs_rms), (rd, rd_rms) = pd.side_errors(R["verts"], R["h"])
    pv = ctx.poisson_mesh(xyz, nrm, depth, scale, trim_cells=0)[0]
    (ps, _), (pd_, _) = pd.side_errors(pv, st["h"])
    print("setup %s depth %d: sparse side max %.4f h (rms %.4f), restatement %.4f (%.4f); dense side %.4f (%.4f), restatement %.4f (%.4f); the plain call "
          "%.2f / %.4f; %d faces, %d cycles, %d of %d samples below depth, least %.3f"
          % (name, depth, gs, gs_rms, rs, rs_rms, gd, gd_rms, rd, rd_rms, ps, pd_, len(f), st["cycles"], st["n_below_depth"], st["n_valid"], st["min_sample_depth"]))
    c = v[f].astype(np.float64) - pr.SPHERE_C
    volume = np.einsum("ij,ij->i", c[:, 0], np.cross(c[:, 1], c[:, 2])).sum() / 6.0              # > 0: the faces look outward
    assert st["converged"] and pr.manifold_report(v, f) == CLOSED and 0.9 < volume / (4.0 / 3.0 * np.pi * pr.SPHERE_R ** 3) < 1.1
    assert abs(gs - rs) <= 0.01 and abs(gd - rd) <= 0.01
    assert gs < 1.0 < ps


def test_repeatable_and_apart_from_the_plain_call(ctx):
    xyz, nrm = samples_of("B")
    p0 = ctx.poisson_mesh(xyz, nrm, 5, trim_cells=2)
    w0 = ctx.poisson_mesh_weighted(xyz, nrm, 5, trim_cells=2, samples_per_node=2.0)
    p1 = ctx.poisson_mesh(xyz, nrm, 5, trim_cells=2)
    w1 = ctx.poisson_mesh_weighted(xyz, nrm, 5, trim_cells=2, samples_per_node=2.0)
    assert same_bits(p0[0], p1[0]) and same_bits(p0[1], p1[1]) and p0[2] == p1[2]
    assert same_bits(w0[0], w1[0]) and same_bits(w0[1], w1[1]) and w0[2] == w1[2]
    assert len(w0[1]) > 1000 and not same_bits(w0[0], p0[0])
    r0, r1 = ctx.poisson_rhs_weighted(xyz, nrm, 5), ctx.poisson_rhs_weighted(xyz, nrm, 5)
    assert all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(r0, r1))


# ---- 5: refusals and empty inputs -----------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    xyz, nrm = random_cloud(300, 3)
    for kw, word in ((dict(kernel_depth=2), "kernel_depth"), (dict(kernel_depth=6), "kernel_depth"), (dict(kernel_depth=-1), "kernel_depth"),
                     (dict(samples_per_node=0.0), "samples_per_node"), (dict(samples_per_node=-2.0), "samples_per_node"),
                     (dict(samples_per_node=float("nan")), "samples_per_node"), (dict(samples_per_node=float("inf")), "samples_per_node"),
                     (dict(depth=4), "depth"), (dict(scale=0.5), "scale"), (dict(trim_cells=-1), "trim_cells"), (dict(max_cycles=0), "max_cycles")):
        with pytest.raises(RsmError, match=word):
            ctx.poisson_mesh_weighted(xyz, nrm, **{**dict(depth=5), **kw})
    for kw, word in ((dict(kernel_depth=2), "kernel_depth"), (dict(samples_per_node=0.0), "samples_per_node")):
        with pytest.raises(RsmError, match=word):
            ctx.poisson_rhs_weighted(xyz, nrm, 5, **kw)
    for bad in (np.nan, np.inf, -np.inf):
        din = np.full(300, 4.0)
        din[299] = bad
        with pytest.raises(RsmError, match=r"depth_in\[299\]"):
            ctx.poisson_rhs_weighted(xyz, nrm, 5, depth_in=din)
    prm, dpr = _lib.PoissonParams(5, 1.1, 0.5, 1, 0), _lib.PoissonDensityParams(0, 2.0)
    nv, nf = C.c_int64(), C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = ctx._lib
    assert lib.rsm_poisson_mesh_weighted(ctx._h, p(xyz), p(nrm), 300, C.byref(prm), None, C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_poisson_mesh_weighted(ctx._h, p(xyz), p(nrm), 300, None, C.byref(dpr), C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_poisson_mesh_weighted(ctx._h, None, p(nrm), 300, C.byref(prm), C.byref(dpr), C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_poisson_mesh_weighted(ctx._h, p(xyz), p(nrm), 300, C.byref(prm), C.byref(dpr), None, C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_poisson_mesh_weighted_device(ctx._h, None, None, 300, C.byref(prm), C.byref(dpr), C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_stage_poisson_rhs_weighted(ctx._h, p(xyz), p(nrm), 300, C.byref(prm), C.byref(dpr), None, None, None, None, None, None, None, None) == _lib.RSM_E_INVALID


def test_nothing_to_mesh(ctx):
    xyz, nrm = random_cloud(64, 4)
    same = np.tile(xyz[:1], (64, 1))
    for x, n, valid in ((np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), 0), (np.tile(BAD_X, (3, 1)), np.tile(BAD_N, (3, 1)), 0), (same, nrm, 64)):
        v, f, st = ctx.poisson_mesh_weighted(x, n, 5)
        assert len(v) == 0 and len(f) == 0 and st["status"] == 0 and st["n_valid"] == valid and st["n_invalid"] == len(x) - valid
        assert st["h"] == 0.0 and st["weight_sum"] == 0.0 and st["n_below_depth"] == 0
        grid, b, occ, counts, rho, w, d = ctx.poisson_rhs_weighted(x, n, 5)
        assert grid[3] == 0.0 and not b.any() and not occ.any() and counts == (valid, len(x) - valid) and not rho.any() and not w.any() and not d.any()


# ---- 6: API and CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cloud_optimization_mesh_with_samples_per_node(ctx):
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
    pv, pf, pst = opt.mesh(depth=6)
    ev, ef, est = ctx.poisson_mesh(sx, sn, 6)
    assert same_bits(pv, ev) and same_bits(pf, ef) and pst == est and "kernel_depth" not in pst          # None is the plain call
    v, f, st = opt.mesh(depth=6, samples_per_node=2)
    assert opt.mesh_result[0] is v and opt.mesh_grid_step == st["h"]
    wv, wf, wst = ctx.poisson_mesh_weighted(sx, sn, 6, samples_per_node=2.0)
    print("run() -> mesh(samples_per_node=2): %d faces (plain %d); %d of %d samples below depth 6, least %.3f" % (len(f), len(pf), st["n_below_depth"], st["n_valid"], st["min_sample_depth"]))
    assert same_bits(v, wv) and same_bits(f, wf) and st == wst and len(f) > 1000 and not same_bits(v, pv)
    v3, f3, st3 = opt.mesh(depth=6, samples_per_node=3, kernel_depth=5)
    assert st["kernel_depth"] == 4 and st3["kernel_depth"] == 5 and not same_bits(v3, v)
    cv, cf, cst = opt.clean_mesh()                                                                          # the later stages run on the result
    assert cst["n_faces_in"] == len(f3) and 0 < len(cf) <= len(f3)


def test_cli_mesh_samples_per_node(ctx, tmp_path, capsys):
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
    assert main(base + ["--mesh", "--mesh-out", root + "plain.ply"]) == 0
    plain = norm(capsys.readouterr().out)
    assert "samples per node" not in plain
    pv, pf = pr.read_ply_mesh(root + "plain.ply")
    blob = open(root + "bigcloud.ply", "rb").read()
    rec = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], "<f4").reshape(-1, 7)
    sx, sn = rec[:, :3].copy(), rec[:, 3:].copy()
    assert main(base + ["--mesh-samples-per-node"]) == 0                                                   # bare: mesh.bat's 2; implies --mesh
    out = norm(capsys.readouterr().out)
    v, f = pr.read_ply_mesh(root + "bigmesh.ply")
    ev, ef, est = ctx.poisson_mesh_weighted(sx, sn, 7, samples_per_node=2.0)
    assert same_bits(v, ev) and np.array_equal(f, ef) and len(f) > 1000 and not same_bits(v, pv)
    lines = out.splitlines()
    assert lines[-2].startswith("Mesh samples per node 2: density on 2^5 nodes, %d of %d samples" % (est["n_below_depth"], est["n_valid"]))
    assert lines[-1] == "%d vertices, %d faces -> %sbigmesh.ply" % (len(v), len(f), root)
    assert main(base + ["--mesh-samples-per-node", "3", "--mesh-kernel-depth", "4", "--mesh-out", root + "m3.ply"]) == 0
    capsys.readouterr()
    e3 = ctx.poisson_mesh_weighted(sx, sn, 7, samples_per_node=3.0, kernel_depth=4)
    assert same_bits(pr.read_ply_mesh(root + "m3.ply")[0], e3[0])
    assert main(base + ["--mesh-samples-per-node", "0"]) == 1
    assert "samples_per_node" in capsys.readouterr().out
