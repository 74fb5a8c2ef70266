"""Development aid: rsm_mesh_subdivide_device (subdiv.mlx's Loop subdivision) on C3's depth-9 mesh after the density trim, the
clean-up and the closing of its holes -- built as tests/tools/meshdecimate_bench.py builds it -- and on that mesh decimated to --target faces:
3 iterations at thr = 0 and at --fraction of the box diagonal, timed with hipEvents after a warm-up; per iteration from calls with
iterations = 1, 2, 3 (the differences), with the bytes an iteration has to move set against the HBM rate; rsm_mesh_decimate_device and
rsm_mesh_clean_device on the same mesh for scale.

python tests/tools/meshsubdivide_bench.py [--pairs 10] [--reps 3] [--depth 9] [--target 100000] [--iterations 3] [--fraction 0.01] [--mls-radius 8]
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/meshsubdivide_bench.py --reps 1 --only-final  (a run of its own)
python tests/tools/meshsubdivide_bench.py --analyze DIR
    reads that run's *kernel_trace.csv: the per-kernel split of the last subdivision call.

The bytes of one iteration on nv vertices, nf faces, ne unique edges, s of them split, nf' faces out (what has to be read or written at
least once; the sorts' and scans' internal passes are not in it): the faces 12 nf and vertices 12 nv in; the edge table's keys and values
written and read sorted 2 x 12 x 3 nf and the corner lists' 2 x 8 x 3 nf; flags, ranks, the split list and the new-vertex entries 4 x 4 x 3 nf;
counts and offsets 8 nf; the vertex arrays 17 nv; out: 12 (nv + s) + 12 nf'."""
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

HBM_GBS = 8000.0           # MI355X: 8 TB/s peak
GROUPS = (("edges, marks, vertex, count", ("k_sd_edges", "k_sd_marks", "k_sd_vertex", "k_sd_count", "k_sd_totals")), ("odd and even points", ("k_sd_odd", "k_sd_even")),
          ("face emit", ("k_sd_emit",)), ("the sorts", ("radix", "onesweep", "histogram", "sort")), ("the scans", ("scan", "lookback")),
          ("tables", ("k_mesh_edge_keys", "k_mesh_corner_keys", "k_mesh_row_starts", "k_mesh_vertex_box")), ("memsets and copies", ("fillbuffer", "copybuffer")))


def iteration_bytes(nv, nf, nsplit, nf_out):
    return 12 * nf + 12 * nv + (2 * 12 + 2 * 8 + 4 * 4) * 3 * nf + 8 * nf + 17 * nv + 12 * (nv + nsplit) + 12 * nf_out


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
    # the last call: back from the last k_sd_emit over as many k_sd_edges launches as it has iterations, to the validation in front of them
    emits = [i for i, r in enumerate(rows) if "k_sd_emit" in r["Kernel_Name"]]
    if not emits:
        print("no k_sd_emit launch in the trace")
        return 1
    end = emits[-1] + 1
    start = end - 1
    while start > 0 and "k_mc_" not in rows[start - 1]["Kernel_Name"] and "k_md_" not in rows[start - 1]["Kernel_Name"]:
        start -= 1
    per, group = {}, {}
    for r in rows[start:end]:
        name = r["Kernel_Name"]
        m = re.search(r"k_(sd|mesh)_\w+", name)
        if m:
            short = m.group(0)
        elif "rocprim" in name:
            short = "rocprim " + re.sub(r".*rocprim::(ROCPRIM_\w+::)?(detail::)?(\w+).*", r"\3", name)[:40]
        else:
            short = re.sub(r"[(<].*", "", name)[:48]
        t = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        per.setdefault(short, []).append(t)
        g = next((g for g, keys in GROUPS if any(k in (short if m else name.lower()) for k in keys)), "other")
        group[g] = group.get(g, 0.0) + t
    total = sum(sum(v) for v in per.values())
    print("the last subdivision call's kernels: %.3f ms in %d launches, %d iterations" % (total, sum(len(v) for v in per.values()), len(per.get("k_sd_emit", []))))
    for g, t in sorted(group.items(), key=lambda kv: -kv[1]):
        print("  %-30s %9.3f ms  %5.1f %%" % (g, t, 100.0 * t / total))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("    %-56s %6d launches %9.3f ms  %5.1f %%" % (name[:56], len(v), sum(v), 100.0 * sum(v) / total))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--fraction", type=float, default=0.01)
    ap.add_argument("--mls-radius", type=float, default=8.0)
    ap.add_argument("--only-final", action="store_true", help="one 3-iteration call at thr = 0 on the final mesh (for a kernel trace)")
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
    nv0, nf0, _ = ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=0)
    mv = torch.empty((nv0, 3), dtype=torch.float32, device="cuda:0")
    mf = torch.empty((nf0, 3), dtype=torch.int32, device="cuda:0")
    ctx.poisson_last_mesh_device(mv.data_ptr(), mf.data_ptr())
    nv1, nf1, tst = ctx.mesh_trim_device(mv.data_ptr(), nv0, mf.data_ptr(), nf0, ox.data_ptr(), on.data_ptr(), k, args.depth, 1.1)
    del ox, on
    tv = torch.empty((nv1, 3), dtype=torch.float32, device="cuda:0")
    tf = torch.empty((nf1, 3), dtype=torch.int32, device="cuda:0")
    ctx.poisson_last_mesh_device(tv.data_ptr(), tf.data_ptr())
    nv2, nf2, cst = ctx.mesh_clean_device(tv.data_ptr(), nv1, tf.data_ptr(), nf1)
    cv_, cf_, hst = ctx.mesh_close_holes_last(30)
    nv, nf = len(cv_), len(cf_)
    dv = torch.from_numpy(cv_).cuda()
    df = torch.from_numpy(cf_).cuda()
    torch.cuda.synchronize()
    print("poisson depth %d trim 0: %d vertices, %d faces; density trim: %d / %d; clean: %d / %d; close holes: %d / %d (%d loops closed)"
          % (args.depth, nv0, nf0, nv1, nf1, nv2, nf2, nv, nf, hst["loops_closed"]), flush=True)
    del mv, mf, tv, tf
    if args.only_final:
        nvo, nfo, st = ctx.mesh_subdivide_device(dv.data_ptr(), nv, df.data_ptr(), nf, iterations=args.iterations)
        nvo, nfo, st = ctx.mesh_subdivide_device(dv.data_ptr(), nv, df.data_ptr(), nf, iterations=args.iterations)
        print("mesh_subdivide x%d at thr 0: %d / %d -> %d / %d" % (args.iterations, nv, nf, nvo, nfo))
        return 0
    measure(ctx, args, torch, "the final mesh", dv, df, nv, nf, True)
    nvd, nfd, dst = ctx.mesh_decimate_device(dv.data_ptr(), nv, df.data_ptr(), nf, target_faces=args.target)
    dv2 = torch.empty((nvd, 3), dtype=torch.float32, device="cuda:0")
    df2 = torch.empty((nfd, 3), dtype=torch.int32, device="cuda:0")
    ctx.poisson_last_mesh_device(dv2.data_ptr(), df2.data_ptr())
    torch.cuda.synchronize()
    measure(ctx, args, torch, "its decimated form", dv2, df2, nvd, nfd, False)
    return 0


def measure(ctx, args, torch, what, dv, df, nv, nf, with_decimate):
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
    print("---- %s: %d vertices, %d faces" % (what, nv, nf), flush=True)
    for label, kw in (("thr 0", {}), ("thr %g of the diagonal" % args.fraction, dict(threshold_fraction=args.fraction))):
        prev_t, prev = 0.0, (nv, nf, 0)
        for it in range(1, args.iterations + 1):
            (ov, of, st), best, every = timed(lambda: ctx.mesh_subdivide_device(dv.data_ptr(), nv, df.data_ptr(), nf, iterations=it, **kw))
            moved = iteration_bytes(prev[0], prev[1], st["split_edges"] - prev[2], of)
            dt = best[0] - prev_t
            print("mesh_subdivide %s, %d iteration%s: -> %d / %d, %d iterations run, %d edges split; hipEvent %.2f ms (wall %.2f ms; all %s); the last iteration "
                  "%.2f ms for at least %.1f MB = %.0f GB/s, %.1f %% of %.0f GB/s" % (label, it, "" if it == 1 else "s", ov, of, st["iterations"], st["split_edges"], best[0],
                                                                                   best[1], every, dt, moved / 1e6, moved / 1e6 / max(dt, 1e-9), 100.0 * moved / 1e6 / max(dt, 1e-9) / HBM_GBS,
                                                                                   HBM_GBS), flush=True)
            prev_t, prev = best[0], (ov, of, st["split_edges"])
        print("stats: %s" % st, flush=True)
    if with_decimate:
        (ov, of, st), best, every = timed(lambda: ctx.mesh_decimate_device(dv.data_ptr(), nv, df.data_ptr(), nf, target_faces=args.target))
        print("mesh_decimate to %d on the same mesh, for scale: -> %d / %d in %d rounds; hipEvent %.2f ms (wall %.2f ms; all %s)"
              % (args.target, ov, of, st["rounds"], best[0], best[1], every), flush=True)
    (cv, cf, st), best, every = timed(lambda: ctx.mesh_clean_device(dv.data_ptr(), nv, df.data_ptr(), nf))
    print("mesh_clean (5 steps) on the same mesh, for scale: %d / %d -> %d / %d; hipEvent %.2f ms (wall %.2f ms; all %s)" % (nv, nf, cv, cf, best[0], best[1], every),
          flush=True)


if __name__ == "__main__":
    sys.exit(main())
