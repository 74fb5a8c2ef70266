"""Development aid: rsm_mesh_decimate_device (decimation.mlx's quadric edge collapse) on C3's depth-9 mesh after the density
trim, the clean-up and the closing of its holes -- the cloud as tests/tools/poisson_bench.py builds it, meshed at trim_cells = 0, trimmed by
rsm_mesh_trim_last, cleaned by rsm_mesh_clean_last and closed by rsm_mesh_close_holes_last with the scripts' settings, then copied out of the
context into buffers of its own so that every repetition decimates the same input -- taken to --target faces, timed with hipEvents after a
warm-up, with rsm_mesh_clean_device on the same mesh for scale.

python tests/tools/meshdecimate_bench.py [--pairs 10] [--reps 3] [--depth 9] [--target 100000] [--mls-radius 8] [--no-per-round]
    prints the mesh, the stats and the time of the call, and the collapses and faces of every round (from calls with max_rounds = 1, 2, ...).
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/meshdecimate_bench.py --reps 1 --no-per-round  (a run of its own)
python tests/tools/meshdecimate_bench.py --analyze DIR
    reads that run's *kernel_trace.csv: the per-kernel split of the last decimation call, grouped into the sorts, the scans, the cost kernel,
    the selection and the rest."""
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

GROUPS = (("the cost kernel", ("k_md_costs",)), ("the selection", ("k_md_rank", "k_md_m2", "k_md_select", "k_md_apply")),
          ("the sorts", ("radix", "onesweep", "histogram", "sort")), ("the scans", ("scan", "lookback")),
          ("tables", ("k_mesh_edge_keys", "k_mesh_corner_keys", "k_mesh_row_starts", "k_md_heads", "k_md_unique", "k_md_vertex", "k_md_entry_border", "k_md_quadrics")),
          ("memsets and copies", ("fillbuffer", "copybuffer")),
          ("faces and vertices", ("k_md_remap", "k_md_compact", "k_md_distinct", "k_md_used", "k_md_renumber", "k_mesh_iota", "k_mesh_compact")))


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
    # a decimation call: from its k_md_distinct launch (the first kernel of the call) to the k_mc_ launch of the clean-up timed after it, or the end
    starts = [i for i, r in enumerate(rows) if "k_md_distinct" in r["Kernel_Name"]]
    if not starts:
        print("no k_md_distinct launch in the trace")
        return 1
    per, group = {}, {}
    for r in rows[starts[-1]:]:
        name = r["Kernel_Name"]
        if "k_mc_" in name:
            break
        m = re.search(r"k_(md|mesh)_\w+", name)
        if m:
            short = m.group(0)
        elif "rocprim" in name:
            short = "rocprim " + re.sub(r".*rocprim::(ROCPRIM_\w+::)?(detail::)?(\w+).*", r"\3", name)[:40]
        else:
            short = re.sub(r"[(<].*", "", name)[:48]              # the runtime's own fill and copy kernels
        t = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        per.setdefault(short, []).append(t)
        g = next((g for g, keys in GROUPS if any(k in (short if m else name.lower()) for k in keys)), "other")
        group[g] = group.get(g, 0.0) + t
    total = sum(sum(v) for v in per.values())
    print("the last decimation call's kernels: %.3f ms in %d launches, %d rounds" % (total, sum(len(v) for v in per.values()), len(per.get("k_md_costs", []))))
    for g, t in sorted(group.items(), key=lambda kv: -kv[1]):
        print("  %-24s %9.3f ms  %5.1f %%" % (g, t, 100.0 * t / total))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("    %-56s %6d launches %9.3f ms  %5.1f %%" % (name[:56], len(v), sum(v), 100.0 * sum(v) / total))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--mls-radius", type=float, default=8.0)
    ap.add_argument("--no-per-round", action="store_true")
    ap.add_argument("--analyze", default=None)
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze)
    import numpy as np
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
    return measure(ctx, args, np, torch, dv, df, nv, nf)


def measure(ctx, args, np, torch, dv, df, nv, nf):
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
    (ov, of, st), best, every = timed(lambda: ctx.mesh_decimate_device(dv.data_ptr(), nv, df.data_ptr(), nf, target_faces=args.target))
    print("mesh_decimate to %d: %d vertices %d faces -> %d / %d in %d rounds, %d collapses (%.0f a round); hipEvent %.2f ms (wall %.2f ms; all %s)"
          % (args.target, nv, nf, ov, of, st["rounds"], st["collapses"], st["collapses"] / max(st["rounds"], 1), best[0], best[1], every), flush=True)
    print("stats: %s" % st, flush=True)
    if not args.no_per_round:
        prev_c, rows = 0, []
        for r in range(1, st["rounds"] + 1):
            _, f_r, s_r = ctx.mesh_decimate_device(dv.data_ptr(), nv, df.data_ptr(), nf, target_faces=args.target, max_rounds=r)
            rows.append("%d:%d/%d" % (r, s_r["collapses"] - prev_c, f_r))
            prev_c = s_r["collapses"]
        print("per round (round:collapses/faces after): %s" % " ".join(rows), flush=True)
    (cv, cf, st), best, every = timed(lambda: ctx.mesh_clean_device(dv.data_ptr(), nv, df.data_ptr(), nf))
    print("mesh_clean (5 steps) on the same mesh, for scale: %d / %d -> %d / %d; hipEvent %.2f ms (wall %.2f ms; all %s)" % (nv, nf, cv, cf, best[0], best[1], every),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
