"""Development aid: rsm_mesh_color_last (colours of the final mesh from the rig's views) on C3 -- the ten pairs of the
portrait rig through the device path, smoothed by rsm_mls_cloud_device, meshed by rsm_poisson_mesh_device at depth 9 with trim 4 and cleaned
by rsm_mesh_clean_last as tests/tools/meshclean_bench.py does, then coloured from the ten pairs' twenty rectified views
(synth.rectified_views) -- timed with hipEvents after a warm-up.

python tests/tools/meshcolor_bench.py [--pairs 10] [--reps 3] [--depth 9] [--mls-radius 8]
    prints the mesh, the counts of the colouring (the share of vertices that stays uncoloured among them) and the time of a call, per mode.
rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/meshcolor_bench.py --reps 1     (a run of its own)
python tests/tools/meshcolor_bench.py --analyze DIR
    reads that run's *kernel_trace.csv: the split over the k_mcol_* kernels, the corner lists' kernels and sort, and the copies' share is
    what is left of the call."""
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
                m = re.search(r"k_mcol_\w+(<[^>]*>)?|k_mc_validate|k_mesh_(corner_keys|row_starts)", r["Kernel_Name"])
                if m:
                    per.setdefault(m.group(0), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    total = sum(sum(v) for v in per.values())
    print("k_mcol_* kernels, validation and the corner lists' kernels: %.2f ms in %d launches" % (total, sum(len(v) for v in per.values())))
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for mode in (1, 0):
        ctx.mesh_color_last(cams, 2.0 * h, mode=mode)        # warm-up
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            e0.record()
            _, _, st = ctx.mesh_color_last(cams, 2.0 * h, mode=mode)
            e1.record()
            e1.synchronize()
            times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
        best = min(times)
        print("mesh_color mode %d, min_cos 0.2, depth_eps 2 h: %d of %d vertices coloured (%.2f %% uncoloured), %d without a normal, %.2f visible views "
              "per coloured vertex, %d (face, view) items drawn, %d in the big-box tier; hipEvent %.2f ms (wall %.2f ms, with the copy of the colours "
              "to the host; all %s)"
              % (mode, st["coloured"], nv, 100.0 * (nv - st["coloured"]) / max(nv, 1), st["no_normal"], st["visible_views"] / max(st["coloured"], 1),
                 st["items_drawn"], st["items_big_box"], best[0], best[1], ["%.2f" % t[0] for t in times]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
