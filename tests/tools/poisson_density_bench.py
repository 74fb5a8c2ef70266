"""Development aid: rsm_poisson_mesh_weighted_device (the density-adaptive form of the Poisson surface) next to
rsm_poisson_mesh_device in the same run, at depth 9 on C3's merged MLS cloud -- the cloud tests/tools/poisson_bench.py times the plain
call on, built the same way (the ten pairs of the portrait rig through the device path, rsm_filter_last_cloud into one buffer in pair
order, smoothed by rsm_mls_cloud_device) -- timed with hipEvents after a warm-up each.

python tests/tools/poisson_density_bench.py [--pairs 10] [--reps 3] [--depth 9] [--trim 4] [--mls-radius 8] [--samples-per-node 2] [--kernel-depth 0]
    prints for either call samples in, vertices / faces out, cycles, residual and the time of a call; for the weighted one also how many
    samples lie below the finest level.
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/poisson_density_bench.py --reps 1     (a run of its own)
python tests/tools/poisson_density_bench.py --analyze DIR
    reads that run's *kernel_trace.csv: the per-kernel split of the k_pv_* (both calls'), k_pd_* and k_mt_* (the weighted call's) kernels."""
import argparse
import csv
import glob
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

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
                m = re.search(r"k_(pv|pd|mt)_\w+(<[^>]*>)?", r["Kernel_Name"])     # ("(anonymous namespace)::k_pd_splat(float const*, ...)")
                if m:
                    per.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    total = sum(sum(v) for v in per.values())
    print("k_pv_* / k_pd_* / k_mt_* kernels: %.2f ms in %d launches" % (total, sum(len(v) for v in per.values())))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("  %-60s %6d launches %9.3f ms  %5.1f %%" % (name[:60], len(v), sum(v), 100.0 * sum(v) / total))
    return 0


def timed(torch, call, reps):
    """(the last result, the (hipEvent ms, wall ms) of every repetition) after one warm-up call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = call()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        out = call()
        e1.record()
        e1.synchronize()
        times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--trim", type=int, default=4)
    ap.add_argument("--mls-radius", type=float, default=8.0, help="the MLS radius that makes the input, as tests/tools/poisson_bench.py's")
    ap.add_argument("--samples-per-node", type=float, default=2.0, help="mesh.bat: 2, script1.mlx: 3")
    ap.add_argument("--kernel-depth", type=int, default=0)
    ap.add_argument("--analyze", default=None)
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze)
    import torch
    from reconstruction_amd import Context, synth
    ctx = Context(0)
    t0 = time.perf_counter()
    cfgs = [synth.config_c3(pair=p) for p in range(args.pairs)]
    cap = sum(c.width * c.height for c in cfgs)
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
    ox = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
    on = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    oi = torch.empty(n, dtype=torch.int32, device="cuda:0")
    k = ctx.mls_cloud_device(rec.data_ptr(), n, nd.data_ptr(), ox.data_ptr(), on.data_ptr(), oi.data_ptr(), args.mls_radius, 1)
    del rec, nd, oi
    print("merged filtered cloud: %d points; MLS (radius %.1f): %d points" % (n, args.mls_radius, k), flush=True)
    (nv, nf, st), times = timed(torch, lambda: ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=args.trim), args.reps)
    best = min(times)
    print("poisson depth %d trim %d: %d samples (%d not valid) -> %d vertices, %d faces (%d / %d before the trim); %d cycles, residual %.2e, "
          "status %d; hipEvent %.2f ms (wall %.2f ms; all %s)"
          % (args.depth, args.trim, k, st["n_invalid"], nv, nf, st["n_vertices_untrimmed"], st["n_faces_untrimmed"], st["cycles"], st["residual"],
             st["status"], best[0], best[1], ["%.2f" % t[0] for t in times]), flush=True)
    print(digest_line(ctx, nv, nf, st), flush=True)
    (nv, nf, st), times = timed(torch, lambda: ctx.poisson_mesh_weighted_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=args.trim,
                                                                                 samples_per_node=args.samples_per_node, kernel_depth=args.kernel_depth), args.reps)
    best = min(times)
    print("poisson weighted depth %d trim %d samples_per_node %g kernel depth %d: %d of %d samples below depth (least %.3f) -> %d vertices, %d faces "
          "(%d / %d before the trim); %d cycles, residual %.2e, status %d; hipEvent %.2f ms (wall %.2f ms; all %s)"
          % (args.depth, args.trim, args.samples_per_node, st["kernel_depth"], st["n_below_depth"], st["n_valid"], st["min_sample_depth"], nv, nf,
             st["n_vertices_untrimmed"], st["n_faces_untrimmed"], st["cycles"], st["residual"], st["status"], best[0], best[1], ["%.2f" % t[0] for t in times]),
          flush=True)
    print(digest_line(ctx, nv, nf, st), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
