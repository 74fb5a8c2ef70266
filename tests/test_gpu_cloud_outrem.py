"""The radius outlier pass of the cloud filter on the MI355X (csrc/k_filter_outrem.hip; pcl::RadiusOutlierRemoval between the statistical
outlier removal and the normals, CCloudOptimization.cpp:90-96) against tests/outrem_restatement.py, the brute-force restatement of its
definition (tests/test_outrem_cpu.py holds that to hand-worked cases and to scipy): the count alone, integer for integer
(rsm_stage_radius_count: the grid route's kernel and its early stop), the filter with the pass on (kept set and statistics' bits, the
normals by tests/test_gpu_cloud_filter.py's standard), off again, on the pixel lattice of a depth map and on the grid, at its ends, and
through CloudOptimization and the command line.  The setting is the session context's: every test switches it off again."""
import contextlib

import numpy as np
import pytest

import cloud_lattice_fixtures as LF
import cloud_probes as cp
import outrem_restatement as R
from oracle import oracle as orc
from reconstruction_amd import RsmError, synth

pytestmark = pytest.mark.gpu

F32 = np.float32
CAM = np.array([30.0, -20.0, 0.0], F32)
_memo = {}


@contextlib.contextmanager
def outrem(ctx, min_neighbors, radius):
    ctx.set_filter_outrem(min_neighbors, radius)
    try:
        yield
    finally:
        ctx.set_filter_outrem()


def clump():
    """The motivating cloud, its statistical removal by the oracle (k = 8, 1 sigma) and its normals' camera: computed once."""
    if "clump" not in _memo:
        xyz, part = R.clump_cloud()
        keep, _, stats = orc.sor_filter(xyz, 8, 1.0)
        _memo["clump"] = (xyz, part, keep, stats)
    return _memo["clump"]


def check_counts(ctx, xyz, radius, caps=(None,)):
    want = R.radius_counts(xyz, radius)
    for cap in caps:
        got = ctx.radius_count(xyz, radius, cap)
        assert got.dtype == np.int32 and np.array_equal(got, want if cap is None else np.minimum(want, cap)), (radius, cap, int((got != np.minimum(want, cap or R.INT32_MAX)).sum()))
    return want


def check_normals(nrm, xyz_kept, radius, cam):
    """tests/test_gpu_cloud_filter.py's standard for the normals of a filtered cloud, against the oracle on that cloud"""
    nrm_o = orc.cloud_normals(xyz_kept, radius, cam)
    nan_o = np.isnan(nrm_o[:, 0])
    assert np.array_equal(np.isnan(nrm[:, 0]), nan_o)
    ok = ~nan_o
    err = np.abs(nrm[ok, :3] - nrm_o[ok, :3]).max(axis=1)
    assert (err < 1e-6).mean() > 0.999 and err.max() < 1e-3, (float((err < 1e-6).mean()), float(err.max()))
    assert np.abs(nrm[ok, 3] - nrm_o[ok, 3]).max() < 1e-6
    assert np.all(np.einsum("ij,ij->i", nrm[ok, :3], np.asarray(cam, F32)[None] - xyz_kept[ok]) >= 0)
    return int(ok.sum())


# ---- 1. the count -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(R.hand_cases())))
def test_count_of_the_hand_worked_cases(ctx, case):
    name, xyz, radius, want = R.hand_cases()[case]
    assert check_counts(ctx, xyz, radius, (None, 1, 2, R.INT32_MAX)).tolist() == want, name


@pytest.mark.parametrize("radius", [1.0, 2.0, 2.5])
def test_count_on_the_clump_cloud_with_caps(ctx, radius):
    xyz = clump()[0]
    want = check_counts(ctx, xyz, radius, (1, 13, 41, R.INT32_MAX, None))
    assert want[100] == want[101] == 0 and want.max() > 13


@pytest.mark.parametrize("o", [0, 1000.25, -37.7])
@pytest.mark.parametrize("r", [0.5, 2.0, 2.5])
def test_count_across_cell_boundaries(ctx, r, o):
    """Pairs within a few ulps of the radius on either side of a cell boundary of the grid the count walks (boundary_cloud: every (r, o))
    and, where the float cell rule of old put an accepted pair two cells apart, cloud_probes' clusters around such pairs (at the origins
    0 and 1000.25 that rule rounds nothing and the generator finds none -- tests/test_outrem_cpu.py): a lost neighbour is a count one
    short."""
    check_counts(ctx, R.boundary_cloud(r, o), r, (None, 2))
    try:
        xyz, info = cp.radius_probe_cloud(r, o, clusters=40)
    except AssertionError as e:
        assert "no straddling pair" in str(e) and o != -37.7
        return
    assert info["lost"] > 0
    check_counts(ctx, xyz, r, (None, 3))


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_count_at_the_wave_and_block_edges(ctx, n):
    rng = np.random.default_rng(n)
    xyz = (rng.uniform(0.0, 6.0, (n, 3)) + [0.0, 0.0, 40.0]).astype(F32)
    want = check_counts(ctx, xyz, 1.5, (None, 4))
    assert want.min() >= 1 and want.max() > 4


def test_count_in_a_flat_box_and_on_equal_points(ctx):
    rng = np.random.default_rng(7)
    flat = np.stack([rng.uniform(0, 9, 700), np.full(700, 3.25), rng.uniform(50, 58, 700)], 1).astype(F32)
    assert check_counts(ctx, flat, 1.0, (None, 5)).max() > 5
    same = np.tile(np.array([[1.5, -2.0, 33.0]], F32), (257, 1))
    assert check_counts(ctx, same, 0.5, (None, 100)).tolist() == [257] * 257
    nothing = np.full((70, 3), np.nan, F32)
    assert check_counts(ctx, nothing, 0.5).tolist() == [0] * 70


# ---- 2. the filter with the pass on ---------------------------------------------------------------------------------------------------
def test_filter_with_the_pass_on_equals_the_oracle_and_the_restatement(ctx):
    xyz, part, keep_o, (mean_o, std_o, thr_o) = clump()
    S = xyz[keep_o]
    ror = R.radius_keep(S, 40, 2.0)
    with outrem(ctx, 40, 2.0):
        kept, nrm, st = ctx.filter_cloud(xyz, 8, 1.0, 2.5, CAM)
        rep = ctx.filter_last_outrem()
    assert np.array_equal(kept, np.nonzero(keep_o)[0][ror]) and len(kept) == 1428
    assert not (part[kept] == 1).any() and not (part[kept] == 3).any()                 # the clump and the non-finite points are gone
    assert (st["mean"], st["stddev"], st["threshold"]) == (mean_o, std_o, thr_o)      # the statistics stay the first pass's
    assert check_normals(nrm, xyz[kept], 2.5, CAM) == len(kept)
    assert (rep["points_in"], rep["removed"], rep["nonfinite"]) == R.report(S, 40, 2.0) == (1952, 524, 2) and rep["window"] == 0
    with outrem(ctx, 12, 1.0):                                                          # ... and the setting that keeps exactly the clump
        kept, nrm, st = ctx.filter_cloud(xyz, 8, 1.0, 2.5, CAM)
    assert np.array_equal(kept, np.nonzero(part == 1)[0]) and not np.isnan(nrm).any()   # (30 points in one neighbourhood: a normal each)


# ---- 3. on, off, a fresh context -------------------------------------------------------------------------------------------------------
def test_switched_off_the_filter_returns_what_it_returned_before(ctx):
    from reconstruction_amd import Context
    xyz = clump()[0]
    kept0, nrm0, st0 = ctx.filter_cloud(xyz, 8, 1.0, 2.5, CAM)
    with outrem(ctx, 40, 2.0):
        kept1, _, _ = ctx.filter_cloud(xyz, 8, 1.0, 2.5, CAM)
        assert ctx.filter_last_outrem()["points_in"] == len(kept0) > len(kept1)
    fresh = Context(0)
    try:
        for c in (ctx, fresh):
            kept, nrm, st = c.filter_cloud(xyz, 8, 1.0, 2.5, CAM)
            assert kept.tobytes() == kept0.tobytes() and nrm.tobytes() == nrm0.tobytes() and st == st0
            assert c.filter_last_outrem() == dict(points_in=-1, removed=0, window=0, nonfinite=0)
    finally:
        fresh.close()


# ---- 4. the lattice route ---------------------------------------------------------------------------------------------------------------
def _depth_map_run(ctx, m, wmax):
    ctx.set_option("filter_window", 24)   # (the probe finds no window on a sparse map: pinned, as tests/test_gpu_cloud_filter_wide.py pins it)
    ctx.set_option("filter_normals_window", wmax)
    try:
        xyz, kept, nrm, st = ctx.filter_depth_map(m.disp, m.mask, m.img, m.Q, m.scale, m.R, m.T, m.own, m.k, 1.0, 2.5, CAM)
        return xyz, kept, nrm, st, ctx.filter_last_outrem(), ctx.filter_last_info()
    finally:
        ctx.set_option("filter_window", 1)
        ctx.set_option("filter_normals_window", 8)


@pytest.mark.parametrize("min_neighbors,radius", [(12, 2.5), (30, 4.0)])
def test_lattice_route_equals_the_grid_route_and_the_restatement(ctx, min_neighbors, radius):
    """dense_f3000 (a thin sheet at lateral spacing 1: a radius of r units is a window of about r pixels): the count on the pixel lattice,
    then the same call with windows forbidden -- the grid route -- and the restatement on the cloud the call returns.  The second case's
    radius is wider than the normals': the window is asked for the larger of the two."""
    m = LF.dense_f3000(8)
    with outrem(ctx, min_neighbors, radius):
        xyz, kept_l, nrm_l, st_l, rep_l, info_l = _depth_map_run(ctx, m, 8)
        xyz_g, kept_g, nrm_g, st_g, rep_g, info_g = _depth_map_run(ctx, m, 0)
    assert rep_l["window"] > 0 and rep_g["window"] == 0, (rep_l, rep_g)
    assert info_l["normals_window"] == rep_l["window"] and info_g["normals_window"] == 0
    assert xyz.tobytes() == xyz_g.tobytes() and kept_l.tobytes() == kept_g.tobytes() and st_l == st_g
    keep_o, _, (mean_o, std_o, thr_o) = orc.sor_filter(xyz, m.k, 1.0)
    assert (st_l["mean"], st_l["stddev"], st_l["threshold"]) == (mean_o, std_o, thr_o)
    ror = R.radius_keep(xyz[keep_o], min_neighbors, radius)
    assert np.array_equal(kept_l, np.nonzero(keep_o)[0][ror]) and 0.3 * keep_o.sum() < ror.sum() < keep_o.sum()
    want = R.report(xyz[keep_o], min_neighbors, radius)
    assert (rep_l["points_in"], rep_l["removed"], rep_l["nonfinite"]) == want == (rep_g["points_in"], rep_g["removed"], rep_g["nonfinite"])
    assert info_l["kept"] == len(kept_l) == info_g["kept"]
    assert np.array_equal(np.isnan(nrm_l), np.isnan(nrm_g))
    ok = ~np.isnan(nrm_g[:, 0])
    assert ok.sum() > 1000 and np.abs(nrm_l[ok] - nrm_g[ok]).max() < 1e-6


# ---- 5. the ends ------------------------------------------------------------------------------------------------------------------------
def test_ends_of_the_neighbour_number(ctx):
    xyz, part, keep_o, stats_o = clump()
    with outrem(ctx, 0, 2.0):                       # only the non-finite points go
        kept, nrm, st = ctx.filter_cloud(xyz, 8, 1.0, 2.5, CAM)
        rep = ctx.filter_last_outrem()
    assert np.array_equal(kept, np.nonzero(keep_o & (part != 3))[0]) and rep == dict(points_in=1952, removed=2, window=0, nonfinite=2)
    with outrem(ctx, 45, 2.0):                      # the largest count is 45: nothing has more
        kept, nrm, st = ctx.filter_cloud(xyz, 8, 1.0, 2.5, CAM)
        rep = ctx.filter_last_outrem()
    assert len(kept) == 0 and len(nrm) == 0 and (st["mean"], st["stddev"], st["threshold"]) == stats_o
    assert rep == dict(points_in=1952, removed=1952, window=0, nonfinite=2)
    with outrem(ctx, 44, 2.0):
        assert len(ctx.filter_cloud(xyz, 8, 1.0, 2.5, CAM)[0]) == int((R.radius_counts(xyz[keep_o], 2.0) == 45).sum()) > 0
    with outrem(ctx, R.INT32_MAX, 2.0):
        assert len(ctx.filter_cloud(xyz, 8, 1.0, 2.5, CAM)[0]) == 0


def test_empty_clouds(ctx):
    with outrem(ctx, 3, 2.0):
        kept, nrm, st = ctx.filter_cloud(np.zeros((0, 3), F32), 8, 1.0, 2.5, CAM)
        assert len(kept) == 0 and ctx.filter_last_outrem() == dict(points_in=0, removed=0, window=0, nonfinite=0)
        kept, nrm, st = ctx.filter_cloud(np.full((9, 3), np.nan, F32), 8, 1.0, 2.5, CAM)
        assert len(kept) == 0 and ctx.filter_last_outrem() == dict(points_in=9, removed=9, window=0, nonfinite=9)
    assert len(ctx.radius_count(np.zeros((0, 3), F32), 2.0)) == 0


@pytest.mark.parametrize("args,why", [((-1, 2.0), "negative"), ((5, float("nan")), "not finite"), ((5, float("inf")), "not finite"),
                                      ((5, 0.0), "not positive"), ((5, -2.0), "not positive"), ((5, 1e-50), "radius is 0 in float32"),
                                      ((5, 1e-30), "square is 0 in float32"), ((5, 1e30), "square is infinite in float32")])
def test_setter_refuses_by_name_and_keeps_the_setting(ctx, args, why):
    xyz = clump()[0]
    with outrem(ctx, 40, 2.0):
        with pytest.raises(RsmError, match=why) as e:
            ctx.set_filter_outrem(*args)
        assert e.value.code == -1
        assert len(ctx.filter_cloud(xyz, 8, 1.0, 2.5, CAM)[0]) == 1428     # the setting before the refusal still holds


def test_count_refuses_a_cap_below_one_and_a_bad_radius(ctx):
    xyz = clump()[0]
    for cap in (0, -3):
        with pytest.raises(RsmError, match="cap"):
            ctx.radius_count(xyz, 2.0, cap)
    with pytest.raises(RsmError, match="not positive"):
        ctx.radius_count(xyz, 0.0)
    with pytest.raises(ValueError):
        ctx.set_filter_outrem(5, None)


# ---- 6. the front ends --------------------------------------------------------------------------------------------------------------------
def test_cloud_optimization_with_use_outrem(ctx):
    from reconstruction_amd import Camera, CloudOptimization, ManageData, StereoMatching
    cfg = synth.config_small(320, 192, 3, radius=2, pair=4, mask_l0_width=60, border_l0=4)
    res = ctx.match_pair(cfg)
    cam = np.zeros(3, F32)
    kept0, nrm0, _ = ctx.filter_cloud(res.xyz, 100, 1.0, 2.5, cam)
    # the two values, from a sample of the survivors: the radius that holds a dozen points at the median and the median count within it, so
    # that the pass removes about half of this rig's cloud (its points are more than 2 apart: CReconstruction.cpp:18's 50 within 2 leaves none)
    S = res.xyz[kept0].astype(F32)
    d2 = cp.fdist2(S[::40, None, :], S[None])
    rad = float(np.sqrt(np.median(np.partition(d2, 12, axis=1)[:, 12])))
    mn = int(np.median(R.radius_counts(S, rad, queries=S[::40])))
    with outrem(ctx, mn, rad):
        kept1, nrm1, _ = ctx.filter_cloud(res.xyz, 100, 1.0, 2.5, cam)
        rep1 = ctx.filter_last_outrem()
    print("use_outrem: more than %d within %g keeps %d of %d" % (mn, rad, len(kept1), len(kept0)))
    assert 0.1 * len(kept0) < len(kept1) < 0.9 * len(kept0) and rep1["points_in"] == len(kept0)
    top = 1 << (cfg.pyr_levels - 1)
    data = ManageData(cam=[[Camera(camID=0, image=cfg.image[0], mask=cfg.mask[0], CamCenter=cam),
                            Camera(camID=1, image=cfg.image[1], mask=cfg.mask[1], CamCenter=cam)]],
                      m_PyrmNum=cfg.pyr_levels, m_LowestLevelSize=(cfg.width // top, cfg.height // top),
                      m_OriginSize=(cfg.width, cfg.height), rectified=[dict(Q=cfg.Q, R_final=cfg.R_final, T_final=cfg.T_final)])
    try:
        for use, kept, nrm in ((True, kept1, nrm1), (False, kept0, nrm0)):
            opt = CloudOptimization(ctx)
            opt.Init(100, 1, mn, rad, 2.5, data, False)      # (CReconstruction.cpp:18, but for the pass's two values)
            assert (opt.m_outrem_neighbor, opt.m_outrem_radius, opt.use_outrem) == (mn, rad, False)
            opt.use_outrem = use
            sm = StereoMatching(0)
            sm.Init(data, opt, 2, 0.03)
            sm.Verbose = 0
            sm.MatchAllLayer()
            fx, fn = opt.cloud_normals[0]
            assert fx.tobytes() == res.xyz[kept].astype(F32).tobytes() and fn.tobytes() == nrm.tobytes()
            assert opt.stats[0]["outrem"] == (rep1 if use else dict(points_in=-1, removed=0, window=0, nonfinite=0))
    finally:
        ctx.set_filter_outrem()


@pytest.fixture(scope="module")
def cli_config(tmp_path_factory):
    from PIL import Image
    from reconstruction_amd import config as cfgmod
    raw = synth.make_raw_pair(origin=(320, 240), baseline=-150.0)   # (a quarter of the other command-line tests' scene: the restatement is O(n^2))
    tmp = tmp_path_factory.mktemp("outrem_cli")
    root = str(tmp) + "/"
    (tmp / "mask").mkdir()
    for j in range(2):
        Image.fromarray(raw["image"][j][:, :, ::-1]).save(root + "0001_Cam%d.png" % j)   # files are RGB, arrays BGR
        Image.fromarray(raw["mask"][j]).save(root + "mask/0001_Cam%d.png" % j)
    cfgmod.dump_opencv_yaml(root + "calib_camera.yml", {"intrinsic-0": raw["K"][0], "extrinsic-0": raw["E"][0],
                                                         "intrinsic-1": raw["K"][1], "extrinsic-1": raw["E"][1]})
    cfgmod.dump_opencv_yaml(root + "config.yml", {
        "filepath": root, "outfilename": root + "out", "isoutput": 0, "camera_calib_name": "calib_camera.yml",
        "PyrmNum": raw["pyr_levels"], "LowestLevelWidth": raw["lowest"][0], "LowestLevelHeight": raw["lowest"][1],
        "imagelist": ["0001_Cam%d.png" % j for j in range(2)], "masklist": ["mask\\0001_Cam%d.png" % j for j in range(2)],
        "camID": np.array([[0, 1]], np.uint8)})
    # the cloud the pass is handed: what --filter alone leaves
    from reconstruction_amd.__main__ import main
    assert main([root + "config.yml", "--filter", "--out", root + "sor.ply"]) == 0
    return root, _ply_xyz(root + "sor.ply")


def _ply_xyz(path):
    body = open(path, "rb").read().split(b"end_header\n", 1)[1]
    return np.frombuffer(body, dtype=[("xyz", "<f4", 3), ("bgr", "u1", 3), ("n", "<f4", 4)])["xyz"].copy()


@pytest.mark.parametrize("values", [[], ["40", "2"], ["12", "20"]])
def test_cli_outrem(cli_config, capsys, values):
    """--outrem bare (50 within 2, CReconstruction.cpp:18), with two values, and with two that suit this scene (its points are several units
    apart, so the first two settings leave nothing): the line it prints and the cloud it writes against the restatement on what --filter alone leaves."""
    from reconstruction_amd.__main__ import main
    root, S = cli_config
    capsys.readouterr()
    assert main([root + "config.yml", "--outrem"] + values) == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Radius outlier removal")]
    assert len(line) == 1 and line[0].endswith("grid of radius-cells")
    mn, r = (int(values[0]), float(values[1])) if values else (50, 2.0)
    keep = R.radius_counts_tree(S, r) > mn       # (tens of thousands of points: the restatement over a k-d tree's candidates)
    print(line[0], "-- the restatement keeps %d of %d" % (keep.sum(), len(S)))
    assert "more than %d within %g" % (mn, r) in line[0] and "%d points in, %d removed" % (len(S), (~keep).sum()) in line[0]
    assert len(S) > 1000 and _ply_xyz(root + "out.ply").tobytes() == S[keep].tobytes()


@pytest.mark.parametrize("values", [["40"], ["40", "2", "7"], ["forty", "2"], ["-1", "2"], ["40", "0"]])
def test_cli_outrem_refusals(cli_config, capsys, values):
    from reconstruction_amd.__main__ import main
    assert main([cli_config[0] + "config.yml", "--outrem"] + values) == 1
    out = capsys.readouterr().out
    assert "--outrem takes no value or two" in out or "rsm_filter_set_outrem" in out
