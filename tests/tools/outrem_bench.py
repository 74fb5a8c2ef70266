"""Development aid: rsm_filter_last_cloud on the C2 pair's cloud with the radius outlier pass (pcl::RadiusOutlierRemoval, CCloudOptimization.cpp:
90-96; csrc/k_filter_outrem.hip) off and on -- one call between hipEvents after a warm-up, repeated; points in and out, the pass's report
(route, points removed) and a checksum of the output, so that two builds can be held to the same bytes.  --root runs a package from another
tree (the parent commit's, for what the pass's plumbing costs when it is off: such a tree has no setter and only the off case runs).
Run it under rocprofv3 --kernel-trace --stats (a separate run) for the per-kernel split.

python tests/tools/outrem_bench.py [--reps 3] [--neighbors 50] [--radius 2.0] [--root DIR] [--normals-window 8]"""
import argparse
import os
import sys
import zlib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--neighbors", type=int, default=50)
ap.add_argument("--radius", type=float, default=2.0)
ap.add_argument("--normals-window", type=int, default=None, help='option "filter_normals_window" (0: the grid route)')
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
args = ap.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

from reconstruction_amd import Context, synth  # noqa: E402

cfg = synth.config_c2(pair=0)
ctx = Context(0)
ctx.upload_pair(cfg)
ctx.run_pair()
n = ctx.n_points
rec = torch.empty((n, 16), dtype=torch.uint8, device="cuda:0")
nrm = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
if args.normals_window is not None:
    ctx.set_option("filter_normals_window", args.normals_window)
has_pass = hasattr(ctx, "set_filter_outrem")
print("package: %s (%s the pass)" % (os.path.abspath(args.root), "with" if has_pass else "without"), flush=True)


def timed(label):
    ms = []
    for i in range(args.reps + 1):           # the first call is the warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m, st = ctx.filter_last_cloud(rec.data_ptr(), nrm.data_ptr(), n, 100, 1.0, 2.5, (0.0, 0.0, 0.0))
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    crc = zlib.crc32(nrm[:m].cpu().numpy().tobytes(), zlib.crc32(rec[:m].cpu().numpy().tobytes()))
    info = ctx.filter_last_info()
    line = "%s: %d -> %d points, hipEvent ms %s (warm-up %.2f), crc %08x, window pass %d, normals window %d" % (
        label, n, m, " ".join("%.2f" % t for t in ms[1:]), ms[0], crc, info["radius"], info["normals_window"])
    if has_pass:
        r = ctx.filter_last_outrem()
        line += "; pass: %d in, %d removed (%d non-finite), %s" % (r["points_in"], r["removed"], r["nonfinite"],
                                                                   "off" if r["points_in"] < 0 else ("pixel window %d" % r["window"] if r["window"] else "grid of radius-cells"))
    print(line, flush=True)


timed("pass off")
if has_pass:
    ctx.set_filter_outrem(args.neighbors, args.radius)
    timed("pass on (%d, %g)" % (args.neighbors, args.radius))
    ctx.set_filter_outrem()
    timed("pass off again")
