"""GPU multi-view duplicate deletion (csrc/k_dedup.hip; CCloudOptimization::run's isdelete branch, CCloudOptimization.cpp:152-346)
against its numpy restatement (tests/dedup_restatement.py), its host / device entries against each other, the geometry of a
rectified pair, CloudOptimization.run() with isdelete on a rig, the CLI, and bad arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

import dedup_restatement as dr
from reconstruction_amd import Camera, CloudOptimization, StereoMatching, synth

pytestmark = pytest.mark.gpu

TOWARD = [0.0, 0.0, -1.0, 0.0]
AWAY = [0.0, 0.0, 1.0, 0.0]


def cams_of(views):
    """dedup_restatement's view dicts as the m_ImageData.cam the Context entries read."""
    out = []
    for v in views:
        out.append([Camera(camID=0, P=v["P"][0], image=v["image"][0], mask=v["mask"][0], bound=tuple(v["bound"]),
                           CamCenter=np.asarray(v["C"], np.float32)),
                    Camera(camID=1, P=v["P"][1], image=v["image"][1], mask=v["mask"][1])])
    return out


def check(ctx, xyz, nrm, views):
    idx, st = ctx.dedup_cloud(xyz, nrm, cams_of(views))
    ridx, rst = dr.dedup(xyz, nrm, views)
    assert np.array_equal(idx, ridx), (len(idx), len(ridx))
    assert st == rst
    return idx, st


@pytest.mark.parametrize("seed,n,pairs,empty", [(1, 20000, 2, False), (2, 200000, 4, True), (3, 60000, 3, False), (4, 5000, 1, False)])
def test_seeded_clouds_match_the_restatement(ctx, seed, n, pairs, empty):
    xyz, nrm, views = dr.random_scene(seed, n, pairs, empty_pair=empty)
    idx, st = check(ctx, xyz, nrm, views)
    assert 0 < len(idx) < n and st["visited"] > 0
    assert st["count0"] > 0 or n < 10000
    if empty:
        assert st["s1"] > 0


def test_hand_built_scenes_match_the_restatement(ctx):
    v = dr.ray_view()
    v["mask"][0][5, 5] = 128
    v["mask"][0][6, 6] = 0
    v["mask"][1][8, 7] = 0
    w = np.full((5, 5, 3), 128, np.uint8)
    w[0, 0, 0], w[1, 1, 1], w[2, 2, 2], w[3, 3, 0] = 148, 108, 148, 108
    v["image"][0][14:19, 14:19] = w
    v["image"][1][14:19, 14:19] = 255 - w                  # CurrentValue == -1 at pixel (16, 16)
    pts, nrm = [], []
    rng = np.random.default_rng(5)
    for k, z in enumerate(rng.permutation(40) * 2.0 + 3.0):   # a 40-point bucket with runs
        pts.append(dr.on_ray(12, 11, z)); nrm.append(TOWARD if (k // 6) % 2 else AWAY)
    for z in (10.0, 4.0):
        pts.append(dr.on_ray(8, 8, z)); nrm.append(TOWARD)
    for z in (10.0, 30.0, 20.0, 5.0):
        pts.append(dr.on_ray(16, 16, z)); nrm.append(TOWARD)
    pts += [dr.on_ray(5, 5, 10), dr.on_ray(6, 6, 10), dr.on_ray(1, 1, 10), [50, 50, -10], [3, 3, 0], dr.on_ray(20, 20, 7)]
    nrm += [TOWARD, TOWARD, TOWARD, TOWARD, TOWARD, [np.nan, 0, 0, 0]]
    p = dr.on_ray(10, 20, 15)
    pts += [p, p, p]; nrm += [TOWARD, AWAY, TOWARD]
    idx, st = check(ctx, np.float32(pts), np.float32(nrm), [v])
    assert st["s1"] == 3 and st["s2"] == 1 and st["count0"] >= 1


def test_host_and_device_entries_agree(ctx):
    xyz, nrm, views = dr.random_scene(7, 50000, 3)
    cams = cams_of(views)
    idx, st = ctx.dedup_cloud(xyz, nrm, cams)
    n = len(xyz)
    rec = np.zeros((n, 4), np.float32)
    rec[:, :3] = xyz
    rec[:, 3] = np.arange(n).astype(np.uint32).view(np.float32)   # colour bytes: any pattern travels along
    d_rec = torch.from_numpy(rec).cuda()
    d_nrm = torch.from_numpy(np.ascontiguousarray(nrm)).cuda()
    d_idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    o_rec = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    o_nrm = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    m, st2 = ctx.dedup_cloud_device(d_rec.data_ptr(), d_nrm.data_ptr(), n, cams, d_idx.data_ptr(), o_rec.data_ptr(), o_nrm.data_ptr())
    torch.cuda.synchronize()
    assert m == len(idx) and st2 == st
    di = d_idx[:m].cpu().numpy()
    assert np.array_equal(di, idx)
    assert np.array_equal(o_rec[:m].cpu().numpy().view(np.uint32), rec[idx].view(np.uint32))
    assert np.array_equal(o_nrm[:m].cpu().numpy().view(np.uint32), nrm[idx].view(np.uint32))
    m2, st3 = ctx.dedup_cloud_device(d_rec.data_ptr(), d_nrm.data_ptr(), n, cams, d_idx.data_ptr())   # no gather
    assert m2 == m and st3 == st


def _run_rig(ctx, rig, isdelete, radius=10.0):
    data = synth.rig_data(rig)
    opt = CloudOptimization(ctx)
    opt.Init(100, 1, 50, 2, radius, data, isdelete)
    sm = StereoMatching(0)
    sm.Init(data, opt, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    return opt, data


def test_single_rectified_pair_keeps_every_point(ctx):
    """One pair through Rectify, MatchAllLayer and the filter: every point lands back in its own bucket, alone."""
    opt, data = _run_rig(ctx, synth.make_raw_rig(2), True)
    xyz, nrm = opt.cloud_normals[0]
    assert len(xyz) > 1000
    idx, st = ctx.dedup_cloud(xyz, nrm, data.cam)
    assert st["s1"] == 0 and st["s2"] == 0 and st["visited"] == len(xyz)
    assert np.array_equal(idx, np.arange(len(xyz)))


def test_rig_run_with_isdelete(ctx):
    rig = synth.make_raw_rig(3)
    opt, data = _run_rig(ctx, rig, True)
    assert len(opt.cloud_normals) == 2
    rx, rn, ri = opt.run()
    xyz = np.concatenate([c[0] for c in opt.cloud_normals])
    ref = np.concatenate([c[1] for c in opt.cloud_normals])
    ip = opt.indicesptr
    # the restatement on the same merged cloud and views
    ridx, rst = dr.dedup(xyz, ref, dr.views_from_cams(data.cam))
    assert np.array_equal(ip, ridx) and opt.dedup_stats == rst
    assert len(ip) < 0.8 * len(xyz)                         # the pairs' shared surface was there twice
    ox, on, oi = ctx.mls_cloud(xyz[ip], 10.0, 1, ref[ip])
    assert np.array_equal(rx, ox) and np.array_equal(rn, on, equal_nan=True) and np.array_equal(ri, ip[oi])
    opt2, _ = _run_rig(ctx, rig, False)
    fx, _, _ = opt2.run()
    assert len(rx) < len(fx)


def test_cli_isdelete_writes_a_smaller_bigcloud(ctx, tmp_path):
    from PIL import Image
    from reconstruction_amd import config as cfgmod
    from reconstruction_amd.__main__ import main
    rig = synth.make_raw_rig(3)
    root = str(tmp_path) + "/"
    (tmp_path / "mask").mkdir()
    calib = {}
    for c in range(3):
        Image.fromarray(rig["image"][c][:, :, ::-1]).save(root + "0001_Cam%d.png" % c)
        Image.fromarray(rig["mask"][c]).save(root + "mask/0001_Cam%d.png" % c)
        calib["intrinsic-%d" % c], calib["extrinsic-%d" % c] = rig["K"][c], rig["E"][c]
    cfgmod.dump_opencv_yaml(root + "calib_camera.yml", calib)
    cfgmod.dump_opencv_yaml(root + "config.yml", {
        "filepath": root, "outfilename": root + "out", "isoutput": 0, "camera_calib_name": "calib_camera.yml",
        "PyrmNum": rig["pyr_levels"], "LowestLevelWidth": rig["lowest"][0], "LowestLevelHeight": rig["lowest"][1],
        "imagelist": ["0001_Cam%d.png" % c for c in range(3)], "masklist": ["mask\\0001_Cam%d.png" % c for c in range(3)],
        "camID": np.array([[0, 1], [1, 2]], np.uint8)})

    def count(path):
        hdr = open(path, "rb").read().split(b"end_header\n", 1)[0].decode()
        return int(hdr.split("element vertex")[1].split()[0])

    assert main([root + "config.yml", "--mls", "--mls-radius", "10", "--mls-out", root + "all.ply"]) == 0
    assert main([root + "config.yml", "--mls", "--isdelete", "--mls-radius", "10", "--mls-out", root + "dedup.ply"]) == 0
    assert 0 < count(root + "dedup.ply") < count(root + "all.ply")


def test_invalid_arguments(ctx):
    from reconstruction_amd._lib import RSM_E_INVALID, RSM_OK
    lib, h = ctx._lib, ctx._h
    xyz, nrm, views = dr.random_scene(9, 1000, 2)
    cams = cams_of(views)
    vs, keep = ctx.dedup_views(cams)
    idx = np.zeros(1000, np.int32)
    m = C.c_int64()
    st = (C.c_int64 * 4)()
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def call(n=1000, v=vs, npairs=2, x=xyz, i=idx, mo=C.byref(m), s=st):
        return lib.rsm_dedup_cloud(h, P(x), P(nrm), C.c_int64(n), v, C.c_int(npairs), None if i is None else P(i), mo, s)

    assert call() == RSM_OK
    assert call(i=None) == RSM_E_INVALID
    assert call(mo=None) == RSM_E_INVALID
    assert call(s=None) == RSM_E_INVALID
    assert call(npairs=0) == RSM_E_INVALID
    assert call(n=-1) == RSM_E_INVALID
    assert call(n=1 << 31) == RSM_E_INVALID
    b = vs[1].bound0
    saved = (b.XL, b.width)
    b.XL, b.width = 1, b.XR - 1 + 1                    # 1 px from the edge: the 5x5 windows would leave the image
    assert call() == RSM_E_INVALID
    b.XL, b.width = saved[0], saved[1] + 3             # width disagrees with XL..XR
    assert call() == RSM_E_INVALID
    b.XL, b.width = saved
    vs[0].bound0.YR = vs[0].height + 5                 # outside the image
    vs[0].bound0.height = vs[0].bound0.YR - vs[0].bound0.YL + 1
    assert call() == RSM_E_INVALID
    assert lib.rsm_dedup_cloud_device(h, None, None, C.c_int64(10), vs, C.c_int(2), None, None, None, C.byref(m), st) == RSM_E_INVALID
    del keep
