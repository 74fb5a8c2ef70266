"""Moving-least-squares smoothing on the MI355X (rsm_mls_cloud / rsm_mls_cloud_device; CCloudOptimization::run,
CCloudOptimization.cpp:348-389) against the numpy restatement in tests/mls_restatement.py, the host and device entries
against each other, CloudOptimization.run() behind MatchAllLayer, and the CLI's --mls."""
import ctypes as C

import numpy as np
import pytest
import torch

from mls_restatement import mls
from reconstruction_amd import synth

pytestmark = pytest.mark.gpu


def surface_cloud(n, seed, extent=60.0, outliers=200, duplicates=50):
    """A bumpy depth-map-like patch (anisotropic sampling as a perspective camera gives it), far and near outliers,
    exact duplicates, an isolated cluster, and non-finite points (the generator of test_gpu_cloud_filter.py)."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2)) * [extent, 0.7 * extent] - [extent / 2, 0.35 * extent]
    z = 600.0 + 6.0 * np.sin(u[:, 0] / 9.0) * np.cos(u[:, 1] / 7.0) + rng.normal(0, 0.03, n)
    xyz = np.c_[u * (z[:, None] / 600.0), z]
    idx = rng.choice(n, outliers, replace=False)
    xyz[idx] += rng.normal(0, 1.0, (outliers, 3)) * rng.choice([0.5, 3.0, 40.0], (outliers, 1))
    idx = rng.choice(n, duplicates, replace=False)
    xyz[idx] = xyz[rng.choice(n, duplicates)]
    xyz[:30] = [200.0, 150.0, 900.0] + rng.normal(0, 0.2, (30, 3))     # an island of 30 points
    xyz[30:32] = [[-300.0, 10.0, 700.0], [-300.5, 10.0, 700.0]]       # an island below 3 neighbours
    xyz = xyz.astype(np.float32)
    xyz[40:44] = [[np.inf, 1.0, 2.0], [np.nan, np.nan, np.nan], [0.0, -np.inf, 5.0], [1.0, 2.0, np.nan]]
    return xyz


def ref_normals(xyz, seed):
    """Filter-like reference normals: +-z at random, some NaN (those never flip)."""
    rng = np.random.default_rng(seed + 100)
    ref = np.zeros((len(xyz), 4), np.float32)
    ref[:, 2] = rng.choice([-1.0, 1.0], len(xyz))
    ref[:, 0] = rng.normal(0, 0.1, len(xyz))
    ref[rng.choice(len(xyz), 20, replace=False)] = np.nan
    return ref


CLOUDS = [(50000, 1), (6000, 2)]
_cache = {}


def restated(n, seed):
    if (n, seed) not in _cache:
        xyz = surface_cloud(n, seed)
        ref = ref_normals(xyz, seed)
        _cache[(n, seed)] = (xyz, ref, mls(xyz, 2.5, (0, 1, 2), ref))
    return _cache[(n, seed)]


def check_against(gx, gn, gi, emit, rx, rn, sampled=False):
    """The tolerances of the MLS parity: positions 2 float32 ulps (99.9 %) / 1e-3 (all), normals 1e-5 (99.9 %), signs exact,
    curvature 1e-6."""
    if not sampled:
        assert np.array_equal(gi, np.nonzero(emit)[0].astype(np.int32))
    rx, rn = rx[emit], rn[emit]
    assert len(gx) == len(rx)
    fin = np.isfinite(rx).all(1)
    assert np.array_equal(np.isfinite(gx).all(1), fin)
    ulp = np.spacing(np.abs(rx[fin]))
    dx = np.abs(gx[fin].astype(np.float64) - rx[fin].astype(np.float64))
    assert (dx <= 2 * ulp).all(1).mean() >= 0.999, float((dx <= 2 * ulp).all(1).mean())
    assert dx.max() < 1e-3, float(dx.max())
    nf = np.isfinite(rn[:, :3]).all(1)
    assert np.array_equal(np.isfinite(gn[:, :3]).all(1), nf)
    dn = np.abs(gn[nf, :3] - rn[nf, :3]).max(1)
    assert (dn < 1e-5).mean() >= 0.999, float((dn < 1e-5).mean())
    assert np.all(np.einsum("ij,ij->i", gn[nf, :3].astype(np.float64), rn[nf, :3]) > 0)     # the same side after the flip
    assert np.abs(gn[nf, 3] - rn[nf, 3]).max() < 1e-6


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("n,seed", CLOUDS)
def test_mls_equals_the_restatement(ctx, n, seed, order):
    xyz, ref, res = restated(n, seed)
    emit, rx, rn = res[order]
    gx, gn, gi = ctx.mls_cloud(xyz, 2.5, order, ref)
    assert not set(range(30, 32)) & set(gi.tolist()) and not set(range(40, 44)) & set(gi.tolist())
    assert set(range(30)) <= set(gi.tolist())
    check_against(gx, gn, gi, emit, rx, rn)


def _records(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return torch.from_numpy(rec).cuda()


def test_host_and_device_entries_give_the_same_bits(ctx):
    xyz, ref, _ = restated(6000, 2)
    n = len(xyz)
    d_rec, d_ref = _records(xyz), torch.from_numpy(ref).cuda()
    for order in (0, 1, 2):
        for use_ref in (True, False):
            hx, hn, hi = ctx.mls_cloud(xyz, 2.5, order, ref if use_ref else None)
            ox = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            on = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            oi = torch.empty(n, dtype=torch.int32, device="cuda")
            m = ctx.mls_cloud_device(d_rec.data_ptr(), n, d_ref.data_ptr() if use_ref else None, ox.data_ptr(), on.data_ptr(),
                                     oi.data_ptr(), 2.5, order)
            assert m == len(hi)
            assert np.array_equal(oi[:m].cpu().numpy(), hi)
            assert np.array_equal(ox[:m].cpu().numpy(), hx, equal_nan=True)
            assert np.array_equal(on[:m].cpu().numpy(), hn, equal_nan=True)


def test_device_entry_on_filtered_pairs_equals_cloud_optimization_run(ctx):
    """rsm_filter_last_cloud of two pairs, concatenated on the device, then rsm_mls_cloud_device with the filter's normals
    against the reference-shaped CloudOptimization.run() behind StereoMatching.MatchAllLayer.  (m_mls_radius = 40: these
    small synthetic clouds' points lie 12 to 19 units apart, at the reference's 2.5 none has 3 neighbours.)"""
    R = 40.0
    from reconstruction_amd import Camera, CloudOptimization, ManageData, StereoMatching
    cfgs = [synth.config_small(320, 192, 3, radius=2, pair=4, mask_l0_width=60, border_l0=4),
            synth.config_small(320, 192, 3, radius=2, pair=5, mask_l0_width=50, border_l0=4, holes=True)]
    cam = np.array([0.0, 0.0, 0.0], np.float32)
    cap = sum(c.width * c.height for c in cfgs)
    rec = torch.empty((cap, 16), dtype=torch.uint8, device="cuda")
    nd = torch.empty((cap, 4), dtype=torch.float32, device="cuda")
    off = 0
    for cfg in cfgs:
        ctx.match_pair(cfg, want_cloud=False)
        m, _ = ctx.filter_last_cloud(rec[off:].data_ptr(), nd[off:].data_ptr(), cap - off, 100, 1.0, R, cam)
        off += m
    assert off > 20000
    ox = torch.empty((off, 3), dtype=torch.float32, device="cuda")
    on = torch.empty((off, 4), dtype=torch.float32, device="cuda")
    oi = torch.empty(off, dtype=torch.int32, device="cuda")
    m = ctx.mls_cloud_device(rec.data_ptr(), off, nd.data_ptr(), ox.data_ptr(), on.data_ptr(), oi.data_ptr(), R, 1)
    assert 0.5 * off < m <= off
    top = 1 << (cfgs[0].pyr_levels - 1)
    data = ManageData(cam=[[Camera(camID=0, image=c.image[0], mask=c.mask[0], CamCenter=cam),
                            Camera(camID=1, image=c.image[1], mask=c.mask[1], CamCenter=cam)] for c in cfgs],
                      m_PyrmNum=cfgs[0].pyr_levels, m_LowestLevelSize=(cfgs[0].width // top, cfgs[0].height // top),
                      m_OriginSize=(cfgs[0].width, cfgs[0].height),
                      rectified=[dict(Q=c.Q, R_final=c.R_final, T_final=c.T_final) for c in cfgs])
    opt = CloudOptimization(ctx)
    opt.Init(100, 1, 50, 2, R, data, False)          # CReconstruction.cpp:18 (but the radius)
    sm = StereoMatching(0)
    sm.Init(data, opt, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    rx, rn, ri = opt.run()
    assert opt.cloud_ms_normals is not None and len(ri) == m
    assert np.array_equal(oi[:m].cpu().numpy(), ri)
    assert np.array_equal(ox[:m].cpu().numpy(), rx, equal_nan=True)
    assert np.array_equal(on[:m].cpu().numpy(), rn, equal_nan=True)
    # the flip: every output normal agrees with its input point's filter normal
    fn = np.concatenate([c[1] for c in opt.cloud_normals])[ri]
    ok = np.isfinite(fn[:, 0]) & np.isfinite(rn[:, 0])
    assert np.all(np.einsum("ij,ij->i", rn[ok, :3], fn[ok, :3]) >= 0)
    opt2 = CloudOptimization(ctx)
    opt2.Init(100, 1, 50, 2, R, data, True)
    with pytest.raises(ValueError, match="152-346"):
        opt2.run()


def test_cli_mls_writes_bigcloud(ctx, tmp_path):
    from PIL import Image
    from reconstruction_amd import config as cfgmod
    from reconstruction_amd.__main__ import main
    raw = synth.make_raw_pair(baseline=-150.0)
    root = str(tmp_path) + "/"
    (tmp_path / "mask").mkdir()
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
    # (this scene's points are 4.3 units apart: at the reference's 2.5 no point has 3 neighbours)
    assert main([root + "config.yml", "--mls", "--mls-radius", "10"]) == 0
    hdr, body = open(root + "bigcloud.ply", "rb").read().split(b"end_header\n", 1)
    props = [l.split()[-1] for l in hdr.decode().splitlines() if l.startswith("property float")]
    assert props == ["x", "y", "z", "normal_x", "normal_y", "normal_z", "curvature"]
    m = int(hdr.decode().split("element vertex")[1].split()[0])
    rec = np.frombuffer(body, "<f4").reshape(-1, 7)
    assert len(rec) == m
    # the filtered cloud the MLS read (out.ply: xyz, colour, the filter's normals) through the restatement
    fhdr, fbody = open(root + "out.ply", "rb").read().split(b"end_header\n", 1)
    frec = np.frombuffer(fbody, dtype=[("xyz", "<f4", 3), ("bgr", "u1", 3), ("n", "<f4", 4)])
    emit, rx, rn = mls(frec["xyz"], 10.0, (1,), frec["n"])[1]
    assert m == emit.sum() and m > 1000
    check_against(rec[:, :3], rec[:, 3:], None, emit, rx, rn, sampled=True)
    assert main([root + "config.yml", "--mls", "--mls-radius", "10", "--mls-out", root + "other.ply"]) == 0
    assert open(root + "other.ply", "rb").read() == open(root + "bigcloud.ply", "rb").read()


def test_invalid_parameters(ctx):
    from reconstruction_amd._lib import RSM_E_INVALID, RSM_OK, MlsParams
    lib, h = ctx._lib, ctx._h
    xyz = surface_cloud(2000, 4)
    ox, on, oi = np.zeros((2000, 3), np.float32), np.zeros((2000, 4), np.float32), np.zeros(2000, np.int32)
    m = C.c_int64()
    P = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(radius=2.5, order=1, n=2000, outs=(P(ox), P(on), P(oi)), n_out=C.byref(m)):
        prm = MlsParams(radius, order)
        return lib.rsm_mls_cloud(h, P(xyz), C.c_int64(n), None, C.byref(prm), *outs, n_out)

    assert call() == RSM_OK and m.value > 0
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert call(radius=r) == RSM_E_INVALID
    for o in (-1, 3):
        assert call(order=o) == RSM_E_INVALID
    assert call(n=-1) == RSM_E_INVALID
    assert call(n=(1 << 31)) == RSM_E_INVALID
    assert call(outs=(None, P(on), P(oi))) == RSM_E_INVALID
    assert call(outs=(P(ox), None, P(oi))) == RSM_E_INVALID
    assert call(outs=(P(ox), P(on), None)) == RSM_E_INVALID
    assert call(n_out=None) == RSM_E_INVALID
    assert lib.rsm_mls_cloud(h, P(xyz), C.c_int64(2000), None, None, P(ox), P(on), P(oi), C.byref(m)) == RSM_E_INVALID
    prm = MlsParams(2.5, 1)
    assert lib.rsm_mls_cloud_device(h, None, C.c_int64(0), None, C.byref(prm), P(ox), P(on), P(oi), C.byref(m)) == RSM_OK and m.value == 0
    assert call(n=0) == RSM_OK and m.value == 0
    x, nn, i = ctx.mls_cloud(np.zeros((0, 3), np.float32))
    assert len(x) == len(nn) == len(i) == 0


def test_c2_filtered_cloud_against_the_restatement_on_samples(ctx):
    """Full size: the C2 bench pair's filtered cloud (~4.75 M points) on the device, 2 000 sampled queries restated.  Radius 8:
    this rig's points lie 1.25 to 6 units apart, and at the reference's 2.5 only ~3 % of them have 3 neighbours."""
    R = 8.0
    cfg = synth.config_c2(pair=0)
    ctx.upload_pair(cfg)
    ctx.run_pair()
    n = ctx.n_points
    rec = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    nd = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    m, _ = ctx.filter_last_cloud(rec.data_ptr(), nd.data_ptr(), n, 100, 1.0, 2.5, (0.0, 0.0, 0.0))
    assert m > 4_000_000
    ox = torch.empty((m, 3), dtype=torch.float32, device="cuda")
    on = torch.empty((m, 4), dtype=torch.float32, device="cuda")
    oi = torch.empty(m, dtype=torch.int32, device="cuda")
    k = ctx.mls_cloud_device(rec.data_ptr(), m, nd.data_ptr(), ox.data_ptr(), on.data_ptr(), oi.data_ptr(), R, 1)
    assert 0.5 * m < k <= m
    xyz = rec[:m].view(torch.float32)[:, :3].cpu().numpy()
    ref = nd[:m].cpu().numpy()
    gi = oi[:k].cpu().numpy()
    pos = np.full(m, -1, np.int64)
    pos[gi] = np.arange(k)
    q = np.sort(np.random.default_rng(11).choice(m, 2000, replace=False))
    emit, rx, rn = mls(xyz, R, (1,), ref, queries=q)[1]
    assert np.array_equal(pos[q] >= 0, emit)
    sel = pos[q][emit]
    full_emit = np.ones(int(emit.sum()), bool)
    check_against(ox[:k].cpu().numpy()[sel], on[:k].cpu().numpy()[sel], None, full_emit, rx[emit], rn[emit], sampled=True)
