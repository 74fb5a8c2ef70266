"""Development aid: rsm_mesh_clean_device (Laplacian smoothing and clean-up of the Poisson surface) on C3's meshes -- the
ten pairs of the portrait rig through the device path, smoothed by rsm_mls_cloud_device and meshed by rsm_poisson_mesh_device at depth 9
as tests/tools/poisson_bench.py does, once untrimmed and once with trim 4 -- timed with hipEvents after a warm-up.

python tests/tools/meshclean_bench.py [--pairs 10] [--reps 3] [--depth 9] [--mls-radius 8]
    prints, per mesh, vertices / faces in and out, the counts of the clean-up, and the time of a call with 5 steps and with none.
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/meshclean_bench.py --reps 1     (a run of its own)
python tests/tools/meshclean_bench.py --analyze DIR
    reads that run's *kernel_trace.csv: the split over the k_mc_* kernels, the topology layer's (mesh_common.h: k_mesh_edge_keys, k_mesh_iota,
    k_mesh_corner_keys, k_mesh_row_starts, k_mesh_vertex_box; not k_mesh_compact_*, which the Poisson trim launches as well) and rocprim's
    radix sort.  profiles/f10_meshclean_kernel_split.log was made when the pattern was k_mc_* alone: its total lacks k_mesh_edge_keys and
    k_mesh_iota (0.7 % of that log) and is not comparable with this split's to that extent."""
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
    per = {}
    for f in files:
        with open(f, newline="") as fp:
            for r in csv.DictReader(fp):
                m = re.search(r"k_mc_\w+(<[^>]*>)?|k_mesh_(edge_keys|iota|corner_keys|row_starts|vertex_box)", r["Kernel_Name"])
                name = m.group(0) if m else ("rocprim radix sort" if re.search(r"radix|onesweep", r["Kernel_Name"]) else None)
                if name:
                    per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    total = sum(sum(v) for v in per.values())
    print("k_mc_* / k_mesh_* kernels and the radix sorts: %.2f ms in %d launches" % (total, sum(len(v) for v in per.values())))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("  %-40s %6d launches %9.3f ms  %5.1f %%" % (name[:40], len(v), sum(v), 100.0 * sum(v) / total))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
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
    for trim in (0, 4):
        nv, nf, _ = ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=trim)
        dv = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda:0")
        df = torch.empty((max(nf, 1), 3), dtype=torch.int32, device="cuda:0")
        ctx.poisson_last_mesh_device(dv.data_ptr(), df.data_ptr())
        for steps in (5, 0):
            ctx.mesh_clean_device(dv.data_ptr(), nv, df.data_ptr(), nf, smooth_steps=steps)          # warm-up
            times = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0.record()
                ov, of, st = ctx.mesh_clean_device(dv.data_ptr(), nv, df.data_ptr(), nf, smooth_steps=steps)
                e1.record()
                e1.synchronize()
                times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
            best = min(times)
            print("mesh_clean depth %d trim %d, %d steps: %d vertices %d faces -> %d / %d; %d border vertices, %d of %d pieces removed (%d faces), "
                  "%d duplicate %d zero-area %d non-manifold; hipEvent %.2f ms (wall %.2f ms; all %s)"
                  % (args.depth, trim, steps, nv, nf, ov, of, st["border_vertices"], st["components_removed"], st["components"], st["removed_isolated"],
                     st["removed_duplicate"], st["removed_zero_area"], st["removed_nonmanifold"], best[0], best[1], ["%.2f" % t[0] for t in times]),
                  flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
