"""Development aid: rsm_mesh_stitch_last (the views' exposure seams levelled in the mesh colours) on C3 -- the cleaned depth-9
mesh of tests/tools/meshcolor_bench.py and its twenty rectified views -- one call between hipEvents after a warm-up.

python tests/tools/meshstitch_bench.py [--pairs 10] [--reps 3] [--depth 9] [--mls-radius 8] [--lambda 0.01] [--iterations 0]
    prints the mesh, the call's counts and time, and the byte model of a step (below).
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/meshstitch_bench.py --reps 1     (a run of its own)
python tests/tools/meshstitch_bench.py --analyze DIR [--step-bytes N]
    reads that run's *kernel_trace.csv: the split over the k_mst_* kernels and the colouring's, the step kernel's time per step and, with
    the bytes per step the timed run printed, their ratio to 8 TB/s.  That ratio is the rate of a cache-served gather -- x (24 bytes per
    vertex) stays in the Infinity Cache and every row is read once per incidence -- not the rate of an HBM stream."""
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

HBM_BYTES_PER_S = 8e12


def step_bytes(n_vertices, incidences):
    """The algorithmic bytes of one k_mst_step launch: per vertex row (4) and deg (4), its own x, b and d read (3 x 24) and d and x' written
    (2 x 24); per incidence the neighbour's index (4) and its x row (24).  Every vertex takes a thread, coloured or not."""
    return 128 * n_vertices + 28 * incidences


def analyze(path, nbytes):
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        print("no *kernel_trace.csv under %s" % path)
        return 1
    per = {}
    for f in files:
        with open(f, newline="") as fp:
            for r in csv.DictReader(fp):
                m = re.search(r"k_mst_\w+|k_mcol_\w+(<[^>]*>)?|k_mc_validate|k_mesh_(corner_keys|row_starts)", r["Kernel_Name"])
                if m:
                    per.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    total = sum(sum(v) for v in per.values())
    print("k_mst_* and k_mcol_* kernels, validation and the corner lists' kernels: %.2f ms in %d launches" % (total, sum(len(v) for v in per.values())))
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print("  %-40s %6d launches %9.3f ms  %5.1f %%" % (name[:40], len(v), sum(v), 100.0 * sum(v) / total))
    steps = per.get("k_mst_step")
    if steps:
        ms = sum(steps) / len(steps)
        print("k_mst_step: %.4f ms per step (min %.4f, max %.4f)" % (ms, min(steps), max(steps)))
        if nbytes:
            rate = nbytes / (ms * 1e-3)
            print("  %.1f MB of algorithmic bytes per step: %.2f TB/s, %.0f %% of 8 TB/s -- a cache-served gather, not an HBM stream" % (nbytes / 1e6, rate / 1e12,
                                                                                                                                    100.0 * rate / HBM_BYTES_PER_S))
    return 0


def c3_mesh(args):
    """C3's cleaned mesh as the context's last mesh, built as tests/tools/meshcolor_bench.py builds it: (ctx, cams, nv, nf, h)"""
    import torch
    from reconstruction_amd import Camera, Context, synth
    ctx = Context(0)
    cap = 0
    cfgs, cams = [], []
    t0 = time.perf_counter()
    for p in range(args.pairs):
        cfg = synth.config_c3(pair=p)
        cfgs.append(cfg)
        cap += cfg.width * cfg.height
        P0, P1, _ = synth.rectified_views(cfg.Q, cfg.R_final, cfg.T_final)
        cams.append([Camera(camID=2 * p, P=P0, image=cfg.image[0], mask=cfg.mask[0]), Camera(camID=2 * p + 1, P=P1, image=cfg.image[1], mask=cfg.mask[1])])
    print("synthesised %d pairs in %.1f s" % (args.pairs, time.perf_counter() - t0), flush=True)
    rec = torch.empty((cap, 16), dtype=torch.uint8, device="cuda:0")
    nd = torch.empty((cap, 4), dtype=torch.float32, device="cuda:0")
    n = 0
    for cfg in cfgs:
        ctx.upload_pair(cfg)
        ctx.run_pair()
        m, _ = ctx.filter_last_cloud(rec[n:].data_ptr(), nd[n:].data_ptr(), cap - n, 100, 1.0, 2.5, (0.0, 0.0, 0.0))
        n += m
    ox = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
    on = torch.empty((n, 4), dtype=torch.float32, device="cuda:0")
    oi = torch.empty(n, dtype=torch.int32, device="cuda:0")
    k = ctx.mls_cloud_device(rec.data_ptr(), n, nd.data_ptr(), ox.data_ptr(), on.data_ptr(), oi.data_ptr(), args.mls_radius, 1)
    del rec, nd, oi
    print("merged filtered cloud: %d points; MLS (radius %.1f): %d points" % (n, args.mls_radius, k), flush=True)
    nv, nf, pst = ctx.poisson_mesh_device(ox.data_ptr(), on.data_ptr(), k, args.depth, trim_cells=4)
    _, _, cst = ctx.mesh_clean_last()
    nv, nf, h = cst["n_vertices"], cst["n_faces"], pst["h"]
    mb = sum(c.image.nbytes + c.mask.nbytes for pair in cams for c in pair) / 1e6
    print("mesh depth %d trim 4, cleaned: %d vertices, %d faces, h = %.4f; %d views of %d x %d (%.0f MB of images and masks uploaded per call)"
          % (args.depth, nv, nf, h, 2 * len(cams), cfgs[0].width, cfgs[0].height, mb), flush=True)
    return ctx, cams, nv, nf, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--mls-radius", type=float, default=8.0)
    ap.add_argument("--lambda", dest="lam", type=float, default=0.01)
    ap.add_argument("--iterations", type=int, default=0)
    ap.add_argument("--analyze", default=None)
    ap.add_argument("--step-bytes", type=float, default=0.0)
    args = ap.parse_args()
    if args.analyze:
        return analyze(args.analyze, args.step_bytes)
    import torch
    ctx, cams, nv, nf, h = c3_mesh(args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.mesh_stitch_last(cams, 2.0 * h, lam=args.lam, iterations=args.iterations)        # warm-up
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        _, _, st = ctx.mesh_stitch_last(cams, 2.0 * h, lam=args.lam, iterations=args.iterations)
        e1.record()
        e1.synchronize()
        times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
    best = min(times)
    nb = step_bytes(nv, st["incidences"])
    print("mesh_stitch lambda %g, min_cos 0.2, depth_eps 2 h: %d of %d vertices coloured, %d incidences (dmax %d), %d across a seam (%d / %d / %d with "
          "two / one / no term); %d steps, relative residual %.2e, largest change %.2f levels, %d values clamped; hipEvent %.2f ms (wall %.2f ms, with "
          "the copy of the colours to the host; all %s)"
          % (args.lam, st["coloured"], nv, st["incidences"], st["dmax"], st["seam_incidences"], st["seam_two_terms"], st["seam_one_term"], st["seam_no_term"],
             st["steps"], st["rel_residual"], st["max_change"], st["clamped"], best[0], best[1], ["%.2f" % t[0] for t in times]), flush=True)
    print("byte model: %d bytes per step (128 per vertex + 28 per incidence) = %.1f MB; x is %.1f MB" % (nb, nb / 1e6, 24 * nv / 1e6), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
