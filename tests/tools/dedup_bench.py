"""Development aid: rsm_dedup_cloud_device (CCloudOptimization::run's isdelete branch) on C3's merged filtered cloud --
the ten pairs of the portrait rig through the device path (rsm_run_pair + rsm_filter_last_cloud into one buffer, pair order, each
pair's normals turned toward its CamCenter), the views from synth.rectified_views -- timed with hipEvents after a warm-up, the
kept points gathered for rsm_mls_cloud_device.  Prints points in and out, the counters and the bucket-size histogram.  Run it under
rocprofv3 --kernel-trace --stats (a separate run) for the per-kernel split (assign, sort, select, scan / write, gather).

python tests/tools/dedup_bench.py [--pairs 10] [--reps 3]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from reconstruction_amd import Camera, Context, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    ctx = Context(0)
    cap = 0
    cfgs, cams = [], []
    t0 = time.perf_counter()
    for p in range(args.pairs):
        cfg = synth.config_c3(pair=p)
        P0, P1, Cc = synth.rectified_views(cfg.Q, cfg.R_final, cfg.T_final)
        bound = ctx.find_margin(cfg.mask[0], cfg.radius)      # MatchAllLayer's top-level margin of the left view
        cams.append([Camera(camID=2 * p, P=P0, image=cfg.image[0], mask=cfg.mask[0], bound=bound.astuple(), CamCenter=Cc),
                     Camera(camID=2 * p + 1, P=P1, image=cfg.image[1], mask=cfg.mask[1])])
        cfgs.append(cfg)
        cap += cfg.width * cfg.height
    print("synthesised %d pairs in %.1f s" % (args.pairs, time.perf_counter() - t0), flush=True)
    rec = torch.empty((cap, 16), dtype=torch.uint8, device="cuda:0")
    nd = torch.empty((cap, 4), dtype=torch.float32, device="cuda:0")
    n = 0
    for cfg, cam in zip(cfgs, cams):
        ctx.upload_pair(cfg)
        ctx.run_pair()
        m, _ = ctx.filter_last_cloud(rec[n:].data_ptr(), nd[n:].data_ptr(), cap - n, 100, 1.0, 2.5, tuple(float(c) for c in cam[0].CamCenter))
        n += m
    print("merged filtered cloud: %d points" % n, flush=True)
    idx = torch.empty(n, dtype=torch.int32, device="cuda:0")
    orec = torch.empty((n, 16), dtype=torch.uint8, device="cuda:0")
    onrm = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    views, keep = ctx.dedup_views(cams)   # (built once: the timed calls pass the same host images)
    m, st = ctx.dedup_cloud_device(rec.data_ptr(), nd.data_ptr(), n, cams, idx.data_ptr(), orec.data_ptr(), onrm.data_ptr())  # warm-up
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        e0.record()
        m, st = ctx.dedup_cloud_device(rec.data_ptr(), nd.data_ptr(), n, cams, idx.data_ptr(), orec.data_ptr(), onrm.data_ptr())
        e1.record()
        e1.synchronize()
        times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
    best = min(times)
    print("dedup: %d points in, %d out (%.1f %%); s1 %d s2 %d count0 %d visited %d; hipEvent %.2f ms (wall %.2f ms; all %s)"
          % (n, m, 100.0 * m / max(n, 1), st["s1"], st["s2"], st["count0"], st["visited"], best[0], best[1],
             ["%.2f" % t[0] for t in times]), flush=True)
    print("images uploaded per call: %.0f MB" % (sum(c[0].image.nbytes * 2 + c[0].mask.nbytes * 2 for c in cams) / 1e6), flush=True)
    # bucket sizes: loop 1 (:160-192) restated on the host (tests/dedup_restatement.py's float32 rules) on the same cloud
    import dedup_restatement as dr
    xyz = rec[:n].view(torch.float32)[:, :3].cpu().numpy()
    nrm = nd[:n, :3].cpu().numpy()
    best = np.full(n, dr.FLT_MIN, np.float32)
    b = np.zeros(n, np.int16)
    with np.errstate(all="ignore"):
        for i, cam in enumerate(cams):
            cd = cam[0].CamCenter[None, :] - xyz
            val = dr._dot3(nrm, cd) / np.sqrt(dr._dot3(cd, cd))
            upd = best < val
            best[upd] = val[upd]
            b[upd] = i
    keys = []
    for i, cam in enumerate(cams):
        sel = np.nonzero(b == i)[0]
        YL, YR, XL, XR, w, h = cam[0].bound
        ok, X, Y = dr._project(*dr._RT(cam[0].P), xyz[sel])
        x, y = X - XL, Y - YL
        inb = ok & (x >= 0) & (x < w) & (y >= 0) & (y < h)
        on = np.zeros(len(sel), bool)
        on[inb] = cam[0].mask[Y[inb], X[inb]] != 0
        keys.append(i * (1 << 40) + y[on] * w + x[on])
    _, sizes = np.unique(np.concatenate(keys), return_counts=True)
    hist = np.bincount(np.minimum(sizes, 17))
    print("bucket sizes (1, 2, ..., 16, >16): %s; buckets %d, largest %d" % (hist[1:].tolist(), len(sizes), sizes.max()), flush=True)
    del keep, views


if __name__ == "__main__":
    main()
