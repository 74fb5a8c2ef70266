"""Development aid: rsm_poisson_mesh_device (the dense-grid Poisson surface and trim) at depth 9 on C3's merged MLS
cloud -- the ten pairs of the portrait rig through the device path (rsm_run_pair + rsm_filter_last_cloud into one buffer, pair
order, as tests/tools/mls_bench.py builds it), smoothed by rsm_mls_cloud_device -- timed with hipEvents after a warm-up.

python tests/tools/poisson_bench.py [--pairs 10] [--reps 3] [--depth 9] [--trim 4] [--mls-radius 8]
    prints samples in, vertices / faces out, cycles, residual and the time of a call.
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/poisson_bench.py --reps 1     (a run of its own)
python tests/tools/poisson_bench.py --analyze DIR [--depth 9]
    reads that run's *kernel_trace.csv: the per-kernel split of the k_pv_* kernels and the smoother's achieved bytes per second at the
    finest level against its algorithmic bytes (a sweep = both colours = one read and one write of chi, one read of b: 12 N^3 bytes).
--curve writes the residual after every cycle at depths 7, 8 and 9 on the noisy sphere (how the default rel_residual was chosen)."""
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


def analyze(path, depth):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        print("no *kernel_trace.csv under %s" % path)
        return 1
    rows = []
    for f in files:
        with open(f, newline="") as fp:
            rows += list(csv.DictReader(fp))
    per = {}
    fine = []
    n3 = 1 << (3 * depth)
    for r in rows:
        m = re.search(r"k_pv_\w+(<[^>]*>)?", r["Kernel_Name"])     # ("(anonymous namespace)::k_pv_rbgs(float*, ...)")
        if not m:
            continue
        name = m.group(0)
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        per.setdefault(name, []).append(dur)
        if "k_pv_rbgs" in name and int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"]) >= n3 // 2:
            fine.append(dur)
    total = sum(sum(v) for v in per.values())
    print("k_pv_* kernels: %.2f ms in %d launches" % (total, sum(len(v) for v in per.values())))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("  %-60s %6d launches %9.3f ms  %5.1f %%" % (name[:60], len(v), sum(v), 100.0 * sum(v) / total))
    if fine:
        # one colour of a sweep at the finest level: half of the sweep's 12 N^3 algorithmic bytes
        ms = sum(fine) / len(fine)
        print("smoother at depth %d: %d colour passes, %.3f ms each = %.2f TB/s of its algorithmic bytes (6 N^3 = %.2f GB a colour)"
              % (depth, len(fine), ms, 6.0 * n3 / (ms * 1e-3) / 1e12, 6.0 * n3 / 1e9))
    return 0


def curve():
    import poisson_restatement as pr
    from reconstruction_amd import Context
    with Context(0) as ctx:
        for depth in (7, 8, 9):
            xyz, nrm = pr.sphere_samples(20 * 4 ** depth)
            _, b, _, _ = ctx.poisson_rhs(xyz, nrm, depth)
            chi, res, cyc, status, hist = ctx.poisson_solve(b, 1e-12, 60)
            print("depth %d, %d samples: floor %.2e (best of %d cycles)" % (depth, len(xyz), res, cyc))
            print("  residual per cycle: " + " ".join("%.2e" % h for h in hist), flush=True)
    return 0


def digest_line(ctx, nv, nf, st):
    """SHA-256 of the last mesh's vertex bytes, of its face bytes and of the stats (the values in key order as float64): two libraries give
    the same three on the same input or they differ somewhere"""
    import hashlib

    import numpy as np
    v, f = ctx.poisson_last_mesh(nv, nf)
    vec = np.concatenate([np.atleast_1d(np.asarray(st[key], np.float64)).ravel() for key in sorted(st)])
    return "  sha256: vertices %s faces %s stats %s" % tuple(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for a in (v, f, vec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--trim", type=int, default=4)
    ap.add_argument("--mls-radius", type=float, default=8.0,
                    help="the MLS radius that makes the input (the synthetic rig's points lie 1.25 to 6 units apart: 8 keeps most of them)")
    ap.add_argument("--analyze", default=None)
    ap.add_argument("--curve", action="store_true")
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze, args.depth)
    if args.curve:
        return curve()
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
    nv, nf, st = ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=args.trim)   # warm-up
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        nv, nf, st = ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=args.trim)
        e1.record()
        e1.synchronize()
        times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
    best = min(times)
    print("poisson depth %d trim %d: %d samples (%d not valid) -> %d vertices, %d faces (%d / %d before the trim); %d cycles, residual %.2e, "
          "status %d; hipEvent %.2f ms (wall %.2f ms; all %s)"
          % (args.depth, args.trim, k, st["n_invalid"], nv, nf, st["n_vertices_untrimmed"], st["n_faces_untrimmed"], st["cycles"], st["residual"],
             st["status"], best[0], best[1], ["%.2f" % t[0] for t in times]), flush=True)
    print(digest_line(ctx, nv, nf, st), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
