"""Development aid: rsm_mls_cloud_device (CCloudOptimization::run's MLS) on C3's merged filtered cloud -- the ten
pairs of the portrait rig through the device path (rsm_run_pair + rsm_filter_last_cloud into one buffer, pair order) -- timed
with hipEvents after a warm-up.  Prints points in, points out and the mean neighbour count (restated on a sample).  Run it
under rocprofv3 --kernel-trace --stats (a separate run) for the per-kernel split.

python tests/tools/mls_bench.py [--pairs 10] [--reps 3] [--order 1] [--radius 2.5 8]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from reconstruction_amd import Context, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--order", type=int, default=1)
    ap.add_argument("--radius", type=float, nargs="+", default=[2.5, 8.0],
                    help="search radii (2.5: m_mls_radius; the synthetic rig's points lie 1.25 to 6 units apart)")
    args = ap.parse_args()
    ctx = Context(0)
    cap = 0
    cfgs = []
    t0 = time.perf_counter()
    for p in range(args.pairs):
        cfgs.append(synth.config_c3(pair=p))
        cap += cfgs[-1].width * cfgs[-1].height
    print("synthesised %d pairs in %.1f s" % (args.pairs, time.perf_counter() - t0), flush=True)
    rec = torch.empty((cap, 16), dtype=torch.uint8, device="cuda:0")
    nd = torch.empty((cap, 4), dtype=torch.float32, device="cuda:0")
    n = 0
    for cfg in cfgs:
        ctx.upload_pair(cfg)
        ctx.run_pair()
        m, _ = ctx.filter_last_cloud(rec[n:].data_ptr(), nd[n:].data_ptr(), cap - n, 100, 1.0, 2.5, (0.0, 0.0, 0.0))
        n += m
    del cfgs
    print("merged filtered cloud: %d points" % n, flush=True)
    ox = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
    on = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    oi = torch.empty(n, dtype=torch.int32, device="cuda:0")
    xyz = rec[:n].view(torch.float32)[:, :3].cpu().numpy()
    srt = np.argsort(xyz[:, 0], kind="stable")
    xs = xyz[srt]
    q = np.random.default_rng(1).choice(n, 2000, replace=False)
    for radius in args.radius:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        k = ctx.mls_cloud_device(rec.data_ptr(), n, nd.data_ptr(), ox.data_ptr(), on.data_ptr(), oi.data_ptr(), radius, args.order)  # warm-up
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            e0.record()
            k = ctx.mls_cloud_device(rec.data_ptr(), n, nd.data_ptr(), ox.data_ptr(), on.data_ptr(), oi.data_ptr(), radius, args.order)
            e1.record()   # (the call returns after its last kernel: the events bracket it on the device's timeline)
            e1.synchronize()
            times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
        # mean neighbour count: the kernel's float32 radius test on 2 000 sampled points (x-sorted slab)
        r2 = np.float32(radius * radius)
        cnt = []
        for i in q:
            p = xyz[i]
            lo, hi = np.searchsorted(xs[:, 0], [p[0] - radius * 1.001, p[0] + radius * 1.001])
            d = xs[lo:hi] - p
            cnt.append(int((((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r2).sum()))
        cnt = np.array(cnt)
        best = min(times)
        print("mls order %d radius %.2f: %d points in, %d out; hipEvent %.2f ms (wall %.2f ms; all %s); mean neighbours %.1f "
              "(sampled, p50 %d, p99 %d)" % (args.order, radius, n, k, best[0], best[1], ["%.2f" % t[0] for t in times], cnt.mean(),
                                             np.percentile(cnt, 50), np.percentile(cnt, 99)), flush=True)


if __name__ == "__main__":
    main()
