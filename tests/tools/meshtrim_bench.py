"""Development aid: rsm_mesh_trim_device (the density trim of the Poisson surface) on C3's merged MLS cloud and its depth-9
mesh at trim_cells = 0 -- the cloud as tests/tools/poisson_bench.py builds it, the mesh copied out of the context into buffers of its own so
that every repetition trims the same input -- timed with hipEvents after a warm-up.

python tests/tools/meshtrim_bench.py [--pairs 10] [--reps 3] [--depth 9] [--trim T] [--smooth 100] [--island-ratio 0.01] [--mls-radius 8]
    prints the Poisson call's time, then samples, vertices / faces in and out, the statistics and the time of a trim call.  --trim defaults
    to mesh.bat's 7 (at depth 9 the rig's values run from 0, on the surface's closing sheet far from any sample, to about 14).
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/meshtrim_bench.py --reps 1     (a run of its own)
python tests/tools/meshtrim_bench.py --analyze DIR
    reads that run's *kernel_trace.csv: the per-kernel split of the k_mt_* kernels, the sorts and scans between them, and the time of one
    smoothing step."""
import argparse
import csv
import glob
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def analyze(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        print("no *kernel_trace.csv under %s" % path)
        return 1
    rows = []
    for f in files:
        with open(f, newline="") as fp:
            rows += list(csv.DictReader(fp))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # the trim calls: from a k_mt_splat launch to the next k_mesh_compact_verts (or the trace's end); what runs between is the call's
    starts = [i for i, r in enumerate(rows) if "k_mt_splat" in r["Kernel_Name"]]
    if not starts:
        print("no k_mt_splat launch in the trace")
        return 1
    first = starts[-1]                                                        # the last call (after the warm-up)
    per = {}
    for r in rows[first:]:
        m = re.search(r"k_(mt|mesh|mc|pv)_\w+(<[^>]*>)?", r["Kernel_Name"])
        name = m.group(0) if m else ("rocprim " + re.sub(r".*rocprim::(detail::)?(\w+).*", r"\2", r["Kernel_Name"])[:40] if "rocprim" in r["Kernel_Name"] else None)
        if name is None:
            continue
        per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    total = sum(sum(v) for v in per.values())
    print("the last trim call's kernels: %.3f ms in %d launches" % (total, sum(len(v) for v in per.values())))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("  %-60s %6d launches %9.3f ms  %5.1f %%" % (name[:60], len(v), sum(v), 100.0 * sum(v) / total))
    if "k_mt_step" in per:
        print("smoothing: %d steps, %.2f us each" % (len(per["k_mt_step"]), 1e3 * sum(per["k_mt_step"]) / len(per["k_mt_step"])))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--trim", type=float, default=7.0)
    ap.add_argument("--smooth", type=int, default=100)
    ap.add_argument("--island-ratio", type=float, default=0.01)
    ap.add_argument("--mls-radius", type=float, default=8.0)
    ap.add_argument("--analyze", default=None)
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze)
    import torch
    from reconstruction_amd import Context, synth
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
    ox = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
    on = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    oi = torch.empty(n, dtype=torch.int32, device="cuda:0")
    k = ctx.mls_cloud_device(rec.data_ptr(), n, nd.data_ptr(), ox.data_ptr(), on.data_ptr(), oi.data_ptr(), args.mls_radius, 1)
    del rec, nd, oi
    print("merged filtered cloud: %d points; MLS (radius %.1f): %d points" % (n, args.mls_radius, k), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=0)                        # warm-up
    torch.cuda.synchronize()
    e0.record()
    nv, nf, pst = ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=0)
    e1.record()
    e1.synchronize()
    print("poisson depth %d trim 0: %d samples -> %d vertices, %d faces; hipEvent %.2f ms" % (args.depth, k, nv, nf, e0.elapsed_time(e1)), flush=True)
    mv = torch.empty((nv, 3), dtype=torch.float32, device="cuda:0")
    mf = torch.empty((nf, 3), dtype=torch.int32, device="cuda:0")
    ctx.poisson_last_mesh_device(mv.data_ptr(), mf.data_ptr())
    torch.cuda.synchronize()
    trim = args.trim
    kw = dict(smooth_steps=args.smooth, trim=trim, island_ratio=args.island_ratio)
    call = lambda: ctx.mesh_trim_device(mv.data_ptr(), nv, mf.data_ptr(), nf, ox.data_ptr(), on.data_ptr(), k, args.depth, 1.1, **kw)
    call()                                                                                                    # warm-up
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        tv, tf, st = call()
        e1.record()
        e1.synchronize()
        times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
    best = min(times)
    print("mesh_trim depth %d (kernel depth %d), %d steps, trim %.3f, island ratio %g: %d samples, %d vertices, %d faces -> %d vertices, %d faces; "
          "hipEvent %.2f ms (wall %.2f ms; all %s)" % (args.depth, st["kernel_depth"], args.smooth, trim, args.island_ratio, k, nv, nf, tv, tf, best[0], best[1],
                                                       ["%.2f" % t[0] for t in times]), flush=True)
    print("stats: %s" % st, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
