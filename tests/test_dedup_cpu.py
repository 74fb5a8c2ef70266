"""The isdelete branch's restatement (tests/dedup_restatement.py) on hand-built scenes with known answers, the rectified-view
geometry helper against the CPU oracle's cloud, and the new C-ABI entries' declarations and struct layout."""
import ctypes as C
import os
import subprocess

import numpy as np

from dedup_restatement import current_value, dedup, on_ray, ray_view
from oracle import oracle as orc
from reconstruction_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOWARD = [0.0, 0.0, -1.0, 0.0]    # faces the camera at the origin: n.(p - C) < 0
AWAY = [0.0, 0.0, 1.0, 0.0]


def run(pts, nrm, views=None):
    return dedup(np.asarray(pts, np.float32), np.asarray(nrm, np.float32), views or [ray_view()])


def test_singletons_come_out_in_row_then_column_order():
    idx, st = run([on_ray(6, 9, 10), on_ray(5, 9, 10), on_ray(20, 4, 10)], [TOWARD] * 3)
    assert idx.tolist() == [2, 1, 0]
    assert st == dict(s1=0, s2=0, count0=0, visited=3)


def test_size_two_opposite_normals_keeps_both_in_bucket_order():
    idx, st = run([on_ray(8, 8, 20), on_ray(8, 8, 10)], [AWAY, TOWARD])
    assert idx.tolist() == [0, 1] and st["count0"] == 0


def test_size_two_right_mask_decides():
    v = ray_view()
    # right view: pixel (x + t / z, y) with t = -4: z = 10 -> x - 0.4 rounds to 8, z = 4 -> x - 1 = 7
    pts, nrm = [on_ray(8, 8, 10), on_ray(8, 8, 4)], [TOWARD, TOWARD]
    assert current_value(v, 8, 8) > -1
    assert dedup(np.float32(pts), np.float32(nrm), [v])[0].tolist() == [0]
    v["mask"][1][8, 8] = 0                       # the first misses the right mask: the second wins
    idx, st = dedup(np.float32(pts), np.float32(nrm), [v])
    assert idx.tolist() == [1] and st["count0"] == 1
    v["mask"][1][8, 7] = 254                     # both miss: nothing
    idx, st = dedup(np.float32(pts), np.float32(nrm), [v])
    assert idx.tolist() == [] and st["count0"] == 2 and st["visited"] == 1
    v["mask"][1][8, 8] = 255                     # only the second misses: the first
    idx, st = dedup(np.float32(pts), np.float32(nrm), [v])
    assert idx.tolist() == [0] and st["count0"] == 1


def test_anti_correlated_window_loses():
    v = ray_view()
    w = np.full((5, 5, 3), 128, np.uint8)
    w[0, 0, 0], w[1, 1, 1], w[2, 2, 2], w[3, 3, 0] = 128 + 20, 128 - 20, 128 + 20, 128 - 20
    v["image"][0][6:11, 6:11] = w
    v["image"][1][6:11, 6:11] = 255 - w             # vecR = -vecL exactly, norms 40: CurrentValue == -1
    assert current_value(v, 8, 8) == -1.0
    idx, st = dedup(np.float32([on_ray(8, 8, 10), on_ray(8, 8, 4)]), np.float32([TOWARD, TOWARD]), [v])
    assert idx.tolist() == [] and st["count0"] == 0
    # in a run of three the farthest stands in when nothing beats -1
    idx, _ = dedup(np.float32([on_ray(8, 8, 10), on_ray(8, 8, 30), on_ray(8, 8, 20), on_ray(8, 8, 5)]),
                   np.float32([TOWARD] * 4), [v])
    assert idx.tolist() == [1]


def test_three_or_more_runs_of_direction_drop_the_nearest():
    z = [10.0, 40.0, 20.0, 30.0]                 # sorted by distance: 1 (40), 3 (30), 2 (20), 0 (10)
    pts = [on_ray(9, 7, t) for t in z]
    # one run: the group [1, 3] by NCC (the first passing right-mask point: 1), 0 dropped... and 2 too
    idx, _ = run(pts, [TOWARD] * 4)
    assert idx.tolist() == [1]
    # two runs: {1, 3} TOWARD, {2, 0} AWAY -> 1, then the run [2] alone at l = n - 1 -> 2
    idx, _ = run(pts, [AWAY, TOWARD, AWAY, TOWARD])
    assert idx.tolist() == [1, 2]
    # three runs: 1 | 3 | 2, 0 -> 1, 3, 2 (and 0, the nearest, never)
    idx, _ = run(pts, [AWAY, TOWARD, AWAY, AWAY])
    assert idx.tolist() == [1, 3]
    idx, _ = run(pts, [TOWARD, TOWARD, AWAY, TOWARD])
    assert idx.tolist() == [1, 2]
    idx, _ = run(pts, [AWAY, TOWARD, TOWARD, AWAY])        # four runs: 1 | 3 | 2 | 0
    assert idx.tolist() == [1, 3, 2]


def test_equal_distances_keep_bucket_order_and_zero_sorts_last():
    p = on_ray(10, 10, 15)
    idx, _ = run([p, p, p], [TOWARD, AWAY, TOWARD])
    assert idx.tolist() == [0, 1]
    # a candidate AT CamCenter (distance 0; the reference reads current_dist[-1]) sorts after the others: sorted 1, 2, 0, and
    # the run {1, 2} (0's direction test n.0 < 0 is false) gives 1
    v = ray_view(C=on_ray(10, 10, 15))
    idx, _ = dedup(np.float32([on_ray(10, 10, 15), on_ray(10, 10, 25), on_ray(10, 10, 20)]), np.float32([TOWARD] * 3), [v])
    assert idx.tolist() == [1]


def test_a_large_bucket():
    zs = np.arange(1, 41, dtype=np.float64) * 3.0
    rng = np.random.default_rng(3)
    perm = rng.permutation(40)
    pts = [on_ray(12, 11, zs[k]) for k in perm]
    dirs = (np.arange(40)[perm] // 7) % 2      # runs of 7 along the distance order
    nrm = [TOWARD if d else AWAY for d in dirs]
    idx, st = run(pts, nrm)
    far_first = np.argsort(-zs[perm], kind="stable")
    # runs along the distance order: 5, 7, 7, 7, 7, 7 points; each run's farthest wins (every right projection passes)
    assert idx.tolist() == [int(far_first[i]) for i in (0, 5, 12, 19, 26, 33)]
    assert st["visited"] == 1


def test_mask_values_and_counters():
    v = ray_view()
    v["mask"][0][5, 5] = 128                     # 1..254: bucketed, never visited
    v["mask"][0][6, 6] = 0                       # s2
    pts = [on_ray(5, 5, 10), on_ray(6, 6, 10), on_ray(1, 1, 10), on_ray(-3, 2, 10), on_ray(8, 8, 10)]
    idx, st = dedup(np.float32(pts), np.float32([TOWARD] * 5), [v])
    assert idx.tolist() == [4]
    assert st == dict(s1=2, s2=1, count0=0, visited=1)
    # behind the camera: the quotient flips the point out of the bound; z = 0: a non-finite quotient
    idx, st = dedup(np.float32([[50, 50, -10], [3, 3, 0]]), np.float32([TOWARD] * 2), [v])
    assert st["s1"] == 2 and len(idx) == 0


def test_best_pair_first_maximum_facing_away_and_nan_normals_go_to_pair_0():
    a, b = ray_view(seed=1), ray_view(seed=2)               # the same geometry: every value ties
    b["mask"][0][8, 8] = 0                                  # ... a point that went to pair 1 would count in s2
    pts = np.float32([on_ray(8, 8, 10)])
    idx, st = dedup(pts, np.float32([TOWARD]), [a, b])
    assert idx.tolist() == [0] and st["s2"] == 0            # the first maximum: pair 0
    a["mask"][0][8, 8], b["mask"][0][8, 8] = 0, 255
    for n in (AWAY, [np.nan, 0, 0, 0]):                     # nothing exceeds FLT_MIN: pair 0
        idx, st = dedup(pts, np.float32([n]), [a, b])
        assert st["s2"] == 1 and len(idx) == 0
    # a normal aimed at pair 1's centre (0, 0, -100): pair 1, whose pixel is X / (Z + 100)
    c = ray_view(seed=3, C=(0.0, 0.0, -100.0))
    c["P"][0] = np.hstack([np.eye(3), np.array([[0.0], [0.0], [100.0]])])
    p = np.float32([[440.0, 550.0, 10.0]])                  # pixel (4, 5) in pair 1, (44, 55) in pair 0 (outside)
    n = np.zeros((1, 4), np.float32)
    n[0, :3] = (np.float32([0, 0, -100]) - p[0]) / np.linalg.norm(np.float32([0, 0, -100]) - p[0])
    idx, st = dedup(p, n, [ray_view(seed=1), c])
    assert st["s1"] == 0 and idx.tolist() == [0]
    idx, st = dedup(p, n, [ray_view(seed=1), dict(c, bound=(10, 5, 10, 5, -4, -4))])   # pair 1 owns no buckets: s1
    assert st["s1"] == 1 and len(idx) == 0


def test_rectified_views_project_a_matched_cloud_back_onto_its_pixels():
    cfg = synth.config_small(96, 64, 2, radius=2, offset=2, pair=1)
    ref = orc.match_pair(cfg)
    P0, P1, Cc = synth.rectified_views(cfg.Q, cfg.R_final, cfg.T_final)
    assert np.allclose(Cc, cfg.T_final)
    xyz = ref["xyz"][np.isfinite(ref["xyz"]).all(1)]
    assert len(xyz) > 500
    h = np.hstack([xyz, np.ones((len(xyz), 1))])
    q0, q1 = h @ P0.T, h @ P1.T
    x, y = q0[:, 0] / q0[:, 2], q0[:, 1] / q0[:, 2]
    assert np.abs(x - np.rint(x)).max() < 1e-6 and np.abs(y - np.rint(y)).max() < 1e-6
    X, Y = np.rint(x).astype(int), np.rint(y).astype(int)
    key = Y * cfg.width + X
    assert np.all(np.diff(key) > 0)                       # one point per pixel, in DisparityToCloud's row-major order
    d = ref["disparity"][0][Y, X]
    assert np.abs(q1[:, 0] / q1[:, 2] - (X + d)).max() < 1e-6
    assert np.abs(q1[:, 1] / q1[:, 2] - Y).max() < 1e-6


def test_header_binding_and_layout_of_rsm_dedup_view(tmp_path):
    from reconstruction_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rsm.h")).read()
    for name in ("rsm_dedup_cloud", "rsm_dedup_cloud_device"):
        assert name + "(" in hdr and name in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert " T rsm_dedup_cloud\n" in out and " T rsm_dedup_cloud_device\n" in out
    fields = ["P", "cam_center", "bound0", "width", "height", "image", "mask"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsm.h"\nint main(void) {\nprintf("size %zu\\n", sizeof(rsm_dedup_view));\n' +
                   "".join('printf("%s %%zu\\n", offsetof(rsm_dedup_view, %s));\n' % (f, f) for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.DedupView)
    for f in fields:
        assert int(got[f]) == getattr(_lib.DedupView, f).offset, f
