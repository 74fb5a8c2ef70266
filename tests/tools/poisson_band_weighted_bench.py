"""Development aid: rsm_poisson_mesh_banded_weighted_device (the banded Poisson call with the density-adaptive splat) on C3's
merged MLS cloud, built as tests/tools/poisson_band_bench.py builds it, at script1.mlx's settings: depth 10, band_bricks 2, trim_cells 8,
samples_per_node 3.  hipEvents after a warm-up, best of --reps with all of them logged; rsm_poisson_mesh_banded_device (the plain splat on the same
band, profiles/f36_poisson_band_bench.log) is timed in the same run.

python tests/tools/poisson_band_weighted_bench.py [--pairs 10] [--reps 3] [--mls-radius 8] [--depth 10] [--band 2] [--trim 8] [--samples-per-node 3]
    both times, the samples below the finest depth, the vertex and face counts, and the peak of the device memory in use during a weighted call
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/poisson_band_weighted_bench.py --reps 1 --only-weighted   (a run of its own)
python tests/tools/poisson_band_weighted_bench.py --analyze DIR
    reads that run's *kernel_trace.csv: the per-kernel split of the k_pbd_* (this unit's), k_pd_* (the level splat and cascade), k_mt_* (the
    density), k_pb_* (the band's) and k_pv_* (the dense solve's) kernels."""
import argparse
import csv
import glob
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from poisson_band_bench import band_line, timed, with_memory_peak  # noqa: E402
from poisson_bench import digest_line  # noqa: E402


def analyze(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        print("no *kernel_trace.csv under %s" % path)
        return 1
    per = {}
    for f in files:
        with open(f, newline="") as fp:
            for r in csv.DictReader(fp):
                m = re.search(r"k_(pbd|pb|pv|pd|mt)_\w+(<[^>]*>)?", r["Kernel_Name"])
                if m:
                    per.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    total = sum(sum(v) for v in per.values())
    print("k_pbd_* / k_pd_* / k_mt_* / k_pb_* / k_pv_* kernels: %.2f ms in %d launches" % (total, sum(len(v) for v in per.values())))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("  %-40s %6d launches %9.3f ms  %5.1f %%  (%.1f us each)" % (name[:40], len(v), sum(v), 100.0 * sum(v) / total, 1e3 * sum(v) / len(v)))
    return 0


def c3_cloud(ctx, torch, pairs, mls_radius):
    """C3's merged MLS cloud on the device: (xyz [k, 3] float32, normals [k, 4] float32, k)"""
    import time
    from reconstruction_amd import synth
    t0 = time.perf_counter()
    cfgs = [synth.config_c3(pair=p) for p in range(pairs)]
    cap = sum(c.width * c.height for c in cfgs)
    print("synthesised %d pairs in %.1f s" % (pairs, time.perf_counter() - t0), flush=True)
    rec = torch.empty((cap, 16), dtype=torch.uint8, device="cuda:0")
    nd = torch.empty((cap, 4), dtype=torch.float32, device="cuda:0")
    n = 0
    for cfg in cfgs:
        ctx.upload_pair(cfg)
        ctx.run_pair()
        m, _ = ctx.filter_last_cloud(rec[n:].data_ptr(), nd[n:].data_ptr(), cap - n, 100, 1.0, 2.5, (0.0, 0.0, 0.0))
        n += m
    del cfgs
    ox = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
    on = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    oi = torch.empty(n, dtype=torch.int32, device="cuda:0")
    k = ctx.mls_cloud_device(rec.data_ptr(), n, nd.data_ptr(), ox.data_ptr(), on.data_ptr(), oi.data_ptr(), mls_radius, 1)
    del rec, nd, oi
    torch.cuda.empty_cache()
    print("merged filtered cloud: %d points; MLS (radius %.1f): %d points" % (n, mls_radius, k), flush=True)
    return ox, on, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mls-radius", type=float, default=8.0, help="the MLS radius that makes the input, as tests/tools/poisson_bench.py's")
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--band", type=int, default=2)
    ap.add_argument("--trim", type=int, default=8)
    ap.add_argument("--samples-per-node", type=float, default=3.0)
    ap.add_argument("--only-weighted", action="store_true", help="leave the plain banded call and the memory watch out (for a kernel trace)")
    ap.add_argument("--analyze", default=None)
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze)
    import torch
    from reconstruction_amd import Context
    ctx = Context(0)
    ox, on, k = c3_cloud(ctx, torch, args.pairs, args.mls_radius)
    tag = "depth %d band_bricks %d trim %d" % (args.depth, args.band, args.trim)
    if not args.only_weighted:
        plain = lambda: ctx.poisson_mesh_banded_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=args.trim, band_bricks=args.band)
        (nv, nf, st), times = timed(torch, plain, args.reps, warm=args.reps > 1)
        print(band_line("banded " + tag, k, nv, nf, st, times), flush=True)
        print(digest_line(ctx, nv, nf, st), flush=True)
    call = lambda: ctx.poisson_mesh_banded_weighted_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=args.trim, band_bricks=args.band,
                                                           samples_per_node=args.samples_per_node)
    (nv, nf, st), times = timed(torch, call, args.reps, warm=args.reps > 1)
    print(band_line("banded weighted %s samples_per_node %g" % (tag, args.samples_per_node), k, nv, nf, st, times), flush=True)
    print("  density on 2^%d nodes; %d of %d samples below depth %d, least depth %.3f; sum of w %.6g; iso %.6g"
          % (st["kernel_depth"], st["n_below_depth"], st["n_valid"], args.depth, st["min_sample_depth"], st["sum_w"], st["iso"]), flush=True)
    print(digest_line(ctx, nv, nf, st), flush=True)
    if not args.only_weighted:
        _, before, peak = with_memory_peak(torch, call)
        print("  device memory in use: %.2f GB before the call, %.2f GB at its peak (sampled every 2 ms)" % (before / 1e9, peak / 1e9), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
