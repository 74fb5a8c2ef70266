"""Development aid: rsm_mesh_fill_colors_last (the vertices no view sees filled from the colours around them) on C3 -- the
cleaned depth-9 mesh of tests/tools/meshstitch_bench.py after its best-view colouring from the twenty rectified views, where three
vertices in four are uncoloured: a deep front -- one call between hipEvents after a warm-up, once with max_rounds 0 and once with 8.

python tests/tools/meshfill_bench.py [--pairs 10] [--reps 3] [--depth 9] [--mls-radius 8] [--max-rounds 0 8] [--iterations 0]
    prints the mesh, the colouring's counts and, per max_rounds, the call's counts and time.  A repeated call does the same work: the
    filled vertices keep best_view -1, so the known set does not change."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--mls-radius", type=float, default=8.0)
    ap.add_argument("--max-rounds", type=int, nargs="+", default=[0, 8])
    ap.add_argument("--iterations", type=int, default=0)
    args = ap.parse_args()
    import torch
    from meshstitch_bench import c3_mesh
    ctx, cams, nv, nf, h = c3_mesh(args)
    _, _, cst = ctx.mesh_color_last(cams, 2.0 * h, mode=0)
    print("mesh_color mode 0, min_cos 0.2, depth_eps 2 h: %d of %d vertices coloured" % (cst["coloured"], nv), flush=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for cap in args.max_rounds:
        ctx.mesh_fill_colors_last(cap, args.iterations)      # warm-up
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            e0.record()
            _, _, st = ctx.mesh_fill_colors_last(cap, args.iterations)
            e1.record()
            e1.synchronize()
            times.append((e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3))
        best = min(times)
        print("mesh_fill_colors max_rounds %d: %d known, %d filled, %d unreached; L = %d rounds, %d kept incidences (dmax %d); %d steps, "
              "largest change from the front %.2f levels, %d values clamped; hipEvent %.2f ms (wall %.2f ms, with the copy of the colours to the host; all %s)"
              % (cap, st["known"], st["filled"], st["unreached"], st["rounds"], st["incidences"], st["dmax"], st["steps"], st["max_change"],
                 st["clamped"], best[0], best[1], ["%.2f" % t[0] for t in times]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
