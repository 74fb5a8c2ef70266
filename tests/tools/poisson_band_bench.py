"""Development aid: rsm_poisson_mesh_banded_device (the finest level of the Poisson surface on a band of bricks) on C3's merged
MLS cloud -- the cloud tests/tools/poisson_bench.py times the dense call on, built the same way (the ten pairs of the portrait rig through the
device path, rsm_filter_last_cloud into one buffer in pair order, smoothed by rsm_mls_cloud_device) -- timed with hipEvents after a warm-up,
best of --reps with all of them logged.

python tests/tools/poisson_band_bench.py [--pairs 10] [--reps 3] [--mls-radius 8] [--case 1|2|12]
    case 1: the banded call at finest depth 9 (band_bricks 1, trim_cells 4) next to the dense call at depth 9 in the same run: time, bricks,
            iterations, both residuals, the vertex and face counts of both meshes, and the distance of the band's vertices from the dense mesh's
            nearest vertex in h (an upper bound of their distance from that mesh)
    case 2: the banded call at depth 10, band_bricks 2, trim_cells 8 (script1.mlx's OctDepth 10): time, active bricks, iterations, residuals and the
            peak of the device memory in use during a call (sampled every 2 ms through hipMemGetInfo, next to what is in use before the call)
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/poisson_band_bench.py --case 2 --reps 1     (a run of its own)
python tests/tools/poisson_band_bench.py --analyze DIR
    reads that run's *kernel_trace.csv: the per-kernel split of the k_pb_* (the band's) and k_pv_* (the dense solve's) kernels."""
import argparse
import csv
import glob
import os
import re
import sys
import threading
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
                m = re.search(r"k_(pb|pv)_\w+(<[^>]*>)?", r["Kernel_Name"])
                if m:
                    per.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    total = sum(sum(v) for v in per.values())
    print("k_pb_* / k_pv_* kernels: %.2f ms in %d launches" % (total, sum(len(v) for v in per.values())))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("  %-40s %6d launches %9.3f ms  %5.1f %%  (%.1f us each)" % (name[:40], len(v), sum(v), 100.0 * sum(v) / total, 1e3 * sum(v) / len(v)))
    return 0


def timed(torch, call, reps, warm=True):
    """(the last result, the (hipEvent ms, wall ms) of every repetition) after one warm-up call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = call() if warm else None
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


def with_memory_peak(torch, call):
    """(the call's result, bytes in use on the device before it, the most seen in use during it)"""
    free0, total = torch.cuda.mem_get_info()
    least = [free0]
    stop = threading.Event()

    def watch():
        while not stop.is_set():
            least[0] = min(least[0], torch.cuda.mem_get_info()[0])
            time.sleep(0.002)
    t = threading.Thread(target=watch)
    t.start()
    try:
        out = call()
    finally:
        stop.set()
        t.join()
    return out, total - free0, total - least[0]


def band_line(tag, k, nv, nf, st, times):
    best = min(times)
    return ("%s: %d samples -> %d vertices, %d faces (%d / %d before the trim); h %.6g; %d of %d bricks active, %d occupied; coarse %d cycles to %.2e; "
            "band %d iterations from %.3e to %.2e; status %d; hipEvent %.2f ms (wall %.2f ms; all %s)"
            % (tag, k, nv, nf, st["n_vertices_untrimmed"], st["n_faces_untrimmed"], st["h"], st["active_bricks"], (st["N"] // 8) ** 3, st["occupied_bricks"],
               st["coarse_cycles"], st["coarse_residual"], st["iterations"], st["residual_before"], st["residual"], st["status"], best[0], best[1],
               ["%.2f" % t[0] for t in times]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mls-radius", type=float, default=8.0, help="the MLS radius that makes the input, as tests/tools/poisson_bench.py's")
    ap.add_argument("--case", default="12")
    ap.add_argument("--analyze", default=None)
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze)
    import numpy as np
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
    torch.cuda.empty_cache()
    print("merged filtered cloud: %d points; MLS (radius %.1f): %d points" % (n, args.mls_radius, k), flush=True)
    if "1" in args.case:
        (nv, nf, st), times = timed(torch, lambda: ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, 9, trim_cells=4), args.reps)
        best = min(times)
        print("dense depth 9 trim 4: %d samples -> %d vertices, %d faces (%d / %d before the trim); h %.6g; %d cycles, residual %.2e, status %d; "
              "hipEvent %.2f ms (wall %.2f ms; all %s)" % (k, nv, nf, st["n_vertices_untrimmed"], st["n_faces_untrimmed"], st["h"], st["cycles"], st["residual"],
                                                           st["status"], best[0], best[1], ["%.2f" % t[0] for t in times]), flush=True)
        print(digest_line(ctx, nv, nf, st), flush=True)
        dv, _ = ctx.poisson_last_mesh(nv, nf)
        (nv, nf, st), times = timed(torch, lambda: ctx.poisson_mesh_banded_device(ox.data_ptr(), on.data_ptr(), k, 9, trim_cells=4, band_bricks=1), args.reps)
        print(band_line("banded depth 9 band_bricks 1 trim 4", k, nv, nf, st, times), flush=True)
        print(digest_line(ctx, nv, nf, st), flush=True)
        bv, _ = ctx.poisson_last_mesh(nv, nf)
        from scipy.spatial import cKDTree
        d = cKDTree(dv.astype(np.float64)).query(bv.astype(np.float64), workers=8)[0] / st["h"]
        print("  band vertices to the nearest dense-mesh vertex: max %.4f h, mean %.4f h, 99th percentile %.4f h" % (d.max(), d.mean(), np.percentile(d, 99)), flush=True)
    if "2" in args.case:
        call = lambda: ctx.poisson_mesh_banded_device(ox.data_ptr(), on.data_ptr(), k, 10, trim_cells=8, band_bricks=2)
        (nv, nf, st), times = timed(torch, call, args.reps, warm=args.reps > 1)
        print(band_line("banded depth 10 band_bricks 2 trim 8", k, nv, nf, st, times), flush=True)
        print(digest_line(ctx, nv, nf, st), flush=True)
        _, before, peak = with_memory_peak(torch, call)
        print("  device memory in use: %.2f GB before the call, %.2f GB at its peak (sampled every 2 ms)" % (before / 1e9, peak / 1e9), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
