"""Development aid: rsm_mesh_close_holes_device (the closing of the surface's small holes) on C3's depth-9 mesh after the
density trim and the clean-up -- the cloud as tests/tools/poisson_bench.py builds it, meshed at trim_cells = 0, trimmed by
rsm_mesh_trim_last and cleaned by rsm_mesh_clean_last with meshlab.bat's settings, then copied out of the context into buffers of its own so
that every repetition closes the same input -- timed with hipEvents after a warm-up, with rsm_mesh_clean_device on the same mesh for scale.

python tests/tools/meshclose_bench.py [--pairs 10] [--reps 3] [--depth 9] [--max-hole 30] [--mls-radius 8]
    prints the mesh, the histogram of its loops' lengths (from the stage entry), the counts of the call and the times of both calls.
python tests/tools/meshclose_bench.py --synthetic NX [--rings K]
    instead of C3's mesh (whose loops may all be long): the NX x NX plane of tests/meshclose_restatement.py's many_holes (a hole of 3 or 4
    edges in every second cell of every second row) followed by K jittered annuli each of 30 and of 64 inner edges -- the fill at work.
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/meshclose_bench.py --reps 1     (a run of its own)
python tests/tools/meshclose_bench.py --analyze DIR
    reads that run's *kernel_trace.csv: the per-kernel split of the last hole-closing call (k_ch_*, the sort and the scans between them)."""
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
    # a hole-closing call: from the k_mesh_edge_keys launch before a k_ch_border to the next k_mc_ launch (the clean-up timed after it) or the end
    borders = [i for i, r in enumerate(rows) if "k_ch_border" in r["Kernel_Name"]]
    if not borders:
        print("no k_ch_border launch in the trace")
        return 1
    first = borders[-1]
    while first > 0 and "k_mesh_edge_keys" not in rows[first]["Kernel_Name"]:
        first -= 1
    per = {}
    for r in rows[first:]:
        if "k_mc_" in r["Kernel_Name"]:
            break
        m = re.search(r"k_(ch|mesh)_\w+(<[^>]*>)?", r["Kernel_Name"])
        name = m.group(0) if m else ("rocprim " + re.sub(r".*rocprim::(detail::)?(\w+).*", r"\2", r["Kernel_Name"])[:40] if "rocprim" in r["Kernel_Name"] else None)
        if name is None:
            continue
        per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    total = sum(sum(v) for v in per.values())
    print("the last hole-closing call's kernels: %.3f ms in %d launches" % (total, sum(len(v) for v in per.values())))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("  %-60s %6d launches %9.3f ms  %5.1f %%" % (name[:60], len(v), sum(v), 100.0 * sum(v) / total))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--max-hole", type=int, default=30)
    ap.add_argument("--mls-radius", type=float, default=8.0)
    ap.add_argument("--analyze", default=None)
    ap.add_argument("--synthetic", type=int, default=0, metavar="NX")
    ap.add_argument("--rings", type=int, default=1000)
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze)
    import numpy as np
    import torch
    from reconstruction_amd import Context, synth
    ctx = Context(0)
    if args.synthetic:
        return synthetic(ctx, args, np, torch)
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
    nv0, nf0, _ = ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=0)
    mv = torch.empty((nv0, 3), dtype=torch.float32, device="cuda:0")
    mf = torch.empty((nf0, 3), dtype=torch.int32, device="cuda:0")
    ctx.poisson_last_mesh_device(mv.data_ptr(), mf.data_ptr())
    nv1, nf1, tst = ctx.mesh_trim_device(mv.data_ptr(), nv0, mf.data_ptr(), nf0, ox.data_ptr(), on.data_ptr(), k, args.depth, 1.1)
    del ox, on
    tv = torch.empty((nv1, 3), dtype=torch.float32, device="cuda:0")
    tf = torch.empty((nf1, 3), dtype=torch.int32, device="cuda:0")
    ctx.poisson_last_mesh_device(tv.data_ptr(), tf.data_ptr())
    nv, nf, cst = ctx.mesh_clean_device(tv.data_ptr(), nv1, tf.data_ptr(), nf1)
    dv = torch.empty((nv, 3), dtype=torch.float32, device="cuda:0")
    df = torch.empty((nf, 3), dtype=torch.int32, device="cuda:0")
    ctx.poisson_last_mesh_device(dv.data_ptr(), df.data_ptr())
    torch.cuda.synchronize()
    print("poisson depth %d trim 0: %d vertices, %d faces; density trim: %d / %d; clean: %d / %d (%d border vertices, %d non-manifold faces removed)"
          % (args.depth, nv0, nf0, nv1, nf1, nv, nf, cst["border_vertices"], cst["removed_nonmanifold"]), flush=True)
    del mv, mf
    return measure(ctx, args, np, torch, dv, df, nv, nf)


def synthetic(ctx, args, np, torch):
    import meshclose_restatement as mc
    v, f, holes = mc.many_holes(args.synthetic, args.synthetic)
    vs, fs, base = [v], [f], len(v)
    for L in (30, 64):
        av, af = mc.annulus(L)
        for r in range(args.rings):
            vs.append(av + np.float32([3.0 * (r % 100), -5.0 - 5.0 * (r // 100), 10.0 * L]))
            fs.append(af + base)
            base += len(av)
    v, f = np.ascontiguousarray(np.concatenate(vs), np.float32), np.ascontiguousarray(np.concatenate(fs), np.int32)
    print("synthetic: the %d x %d plane with %d holes of 3 or 4 edges, %d annuli each of 30 and 64 inner edges: %d vertices, %d faces"
          % (args.synthetic, args.synthetic, holes, args.rings, len(v), len(f)), flush=True)
    return measure(ctx, args, np, torch, torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), len(v), len(f))


def measure(ctx, args, np, torch, dv, df, nv, nf):
    label, size, nc = ctx.mesh_border_loops(df.cpu().numpy(), nv)
    roots = np.nonzero(label == np.arange(len(label)))[0]
    lengths = size[roots]
    loops = lengths[lengths > 0]
    hist = np.bincount(np.minimum(loops, 65), minlength=66)
    print("border components %d: %d open, %d loops; loop lengths (length: count; 65 = longer): %s"
          % (nc, int((lengths == 0).sum()), len(loops), " ".join("%d:%d" % (L, c) for L, c in enumerate(hist) if c)), flush=True)
    if len(loops):
        print("longest loop %d, median %d; loops of at most %d: %d" % (loops.max(), int(np.median(loops)), args.max_hole, int((loops <= args.max_hole).sum())), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(call):
        call()                                                                                                # warm-up
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            e0.record()
            res = call()
            e1.record()
            e1.synchronize()
            times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
        return res, min(times), ["%.2f" % t[0] for t in times]
    for max_hole in sorted({args.max_hole, 64}):
        (ov, of, st), best, every = timed(lambda: ctx.mesh_close_holes_device(dv.data_ptr(), nv, df.data_ptr(), nf, max_hole))
        print("mesh_close_holes max_hole_size %d: %d vertices %d faces -> %d faces; hipEvent %.2f ms (wall %.2f ms; all %s)" % (max_hole, nv, nf, of, best[0], best[1], every),
              flush=True)
        print("stats: %s" % st, flush=True)
    (cv, cf, st), best, every = timed(lambda: ctx.mesh_clean_device(dv.data_ptr(), nv, df.data_ptr(), nf))
    print("mesh_clean (5 steps) on the same mesh, for scale: %d / %d -> %d / %d; hipEvent %.2f ms (wall %.2f ms; all %s)" % (nv, nf, cv, cf, best[0], best[1], every),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
