"""Known answers for the numpy restatement of the density trim (tests/meshtrim_restatement.py), worked by hand or from the
analytic scene -- the GPU tests (tests/test_gpu_meshtrim.py) hold the kernels to this restatement, these hold the restatement itself.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import meshtrim_restatement as mt

TRI_V = np.float32([[0, 0, 0], [2, 0, 0], [0, 2, 0]])
TRI_F = np.int32([[0, 1, 2]])


def test_binding_lists_the_trim_and_mirrors_its_struct(tmp_path):
    from reconstruction_amd import _lib
    for name in ("rsm_mesh_trim", "rsm_mesh_trim_device", "rsm_mesh_trim_last", "rsm_stage_mesh_density", "rsm_stage_mesh_value_smooth", "rsm_stage_mesh_split"):
        assert name in _lib.PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in _lib.MeshTrimParams._fields_]
    body = 'printf("%zu\\n", sizeof(rsm_mesh_trim_params));\n' + "".join('printf("%%zu\\n", offsetof(rsm_mesh_trim_params, %s));\n' % f for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsm.h"\nint main(void) {\n%sprintf("%%d\\n", RSM_MESH_TRIM_STATS);\nreturn 0; }\n' % body)
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(root, "include"), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.MeshTrimParams) and got[-1] == _lib.MESH_TRIM_STATS
    assert got[1:-1] == [getattr(_lib.MeshTrimParams, f).offset for f in fields]


def test_one_triangle_with_one_corner_below():
    # keep = (1, 1, 0): corner 2 alone.  Edges (0, 2) and (1, 2) are cut half way: vertices 3 = (0, 1, 0), 4 = (1, 1, 0).  The triangle
    # (2, 3, 4) is dropped; the quad (3, 0, 1, 4) has |q1 - q3|^2 = 2 < |q0 - q2|^2 = 5: (3, 0, 4), (0, 1, 4)
    r = mt.split(TRI_V, TRI_F, [8.0, 8.0, 6.0], 7.0)
    assert r["split_faces"].tolist() == [[2, 3, 4], [3, 0, 4], [0, 1, 4]] and r["split_side"].tolist() == [0, 1, 1]
    assert r["split_vertices"].tolist() == [[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 1, 0], [1, 1, 0]]
    assert r["vertices"].tolist() == [[0, 0, 0], [2, 0, 0], [0, 1, 0], [1, 1, 0]] and r["faces"].tolist() == [[2, 0, 3], [0, 1, 3]]
    assert r["src"].tolist() == [0, 0] and r["side"].tolist() == [1, 1] and r["label"].tolist() == [1, 1]
    st = r["stats"]
    assert (st["cut_edges"], st["faces_split"], st["zero_area_triangles"], st["components_kept"], st["components_dropped"]) == (2, 1, 0, 1, 1)
    # areas: D^2 = 8, the triangle is 2 of which 1/2 is dropped
    assert r["q"] == [2 ** 32 // 16, 2 ** 32 // 16, 2 ** 32 // 8] and st["q_total"] == 2 ** 32 // 4


def test_one_triangle_with_one_corner_above():
    # keep = (1, 0, 0): corner 0 alone, vertices 3 = (1, 0, 0) on (0, 1), 4 = (0, 1, 0) on (0, 2); (0, 3, 4) is kept
    r = mt.split(TRI_V, TRI_F, [8.0, 6.0, 6.0], 7.0)
    assert r["split_faces"].tolist()[0] == [0, 3, 4] and r["split_side"].tolist() == [1, 0, 0]
    assert r["split_faces"].tolist()[1:] == [[3, 1, 2], [3, 2, 4]]              # |q1 - q3|^2 = 5 is not below |q0 - q2|^2 = 5
    assert r["vertices"].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]] and r["faces"].tolist() == [[0, 1, 2]]
    # the other orientation keeps its winding
    r = mt.split(TRI_V, TRI_F[:, ::-1], [8.0, 6.0, 6.0], 7.0)
    assert r["split_faces"].tolist()[0] == [0, 4, 3] and r["vertices"].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]] and r["faces"].tolist() == [[0, 2, 1]]


def test_a_vertex_on_the_iso_line_is_kept_and_its_cut_vertices_coincide_with_it():
    r = mt.split(TRI_V, TRI_F, [7.0, 6.0, 6.0], 7.0)
    assert r["split_side"].tolist() == [1, 0, 0]
    assert r["split_vertices"][3:].tolist() == [[0, 0, 0], [0, 0, 0]]            # t = 0 on both edges
    assert r["stats"]["zero_area_triangles"] == 2                               # (0, 3, 4) and the quad's (3, 2, 4)
    assert r["faces"].tolist() == [[0, 1, 2]] and r["vertices"].tolist() == [[0, 0, 0]] * 3
    # all below, all above, a repeated index
    assert mt.split(TRI_V, TRI_F, [6.0, 6.0, 6.9], 7.0)["faces"].shape == (0, 3)
    assert mt.split(TRI_V, TRI_F, [7.0, 7.0, 7.0], 7.0)["faces"].tolist() == [[0, 1, 2]]
    r = mt.split(TRI_V, np.int32([[0, 1, 1], [0, 1, 2]]), [8.0, 8.0, 8.0], 7.0)
    assert r["faces"].tolist() == [[0, 1, 2]] and r["src"].tolist() == [1] and r["stats"]["repeated_index_faces"] == 1


def test_smoothing_by_hand_and_on_a_linear_ramp():
    # one triangle: every vertex has the two others as incidences, once each
    x = mt.value_smooth([3.0, 6.0, 9.0], TRI_F, 1)
    assert x.tolist() == [(3.0 + (6.0 + 9.0)) / 3.0, (6.0 + (9.0 + 3.0)) / 3.0, (9.0 + (3.0 + 6.0)) / 3.0]
    # a repeated-index face is in no list, an unreferenced vertex keeps its value, 0 steps change nothing
    assert mt.value_smooth([1.0, 2.0, 4.0, -0.0], np.int32([[0, 1, 1], [0, 1, 2]]), 3)[3] == 0.0
    assert mt.value_smooth([1.0, 2.0, 4.0], np.int32([[0, 1, 1]]), 5).tolist() == [1.0, 2.0, 4.0]
    assert mt.value_smooth([1.0, 2.0, 4.0], TRI_F, 0).tolist() == [1.0, 2.0, 4.0]
    # an interior edge counts twice, a border edge once
    start, nbr = mt.neighbours(np.int32([[0, 1, 2], [0, 2, 3]]), 4)
    assert nbr[start[0]:start[1]].tolist() == [1, 2, 2, 3] and nbr[start[1]:start[2]].tolist() == [2, 0]
    # the plane: the incidences of an interior vertex are symmetric about it, so a linear ramp stays
    v, f = mt.plane(41, 31)
    x0 = 0.5 * v[:, 0].astype(np.float64) + 0.25 * v[:, 1].astype(np.float64) + 0.1
    x1 = mt.value_smooth(x0, f, 1)
    inner = (v[:, 0] > 0) & (v[:, 0] < 40) & (v[:, 1] > 0) & (v[:, 1] < 30)
    assert np.abs(x1 - x0)[inner].max() < 1e-13 and np.abs(x1 - x0)[~inner].max() > 0.05


def test_the_ramp_is_cut_along_the_straight_line_and_keeps_the_analytic_area():
    v, f = mt.plane(41, 31)
    x = 0.5 * v[:, 0].astype(np.float64) + 0.1                                   # 7 at x = 13.8
    r = mt.split(v, f, x, 7.0)
    cutv = r["split_vertices"][len(v):]
    assert len(cutv) == r["stats"]["cut_edges"] == 30 + 31 and np.abs(cutv[:, 0] - 13.8).max() < 2e-6
    assert r["vertices"][:, 0].min() == cutv[:, 0].min() and r["stats"]["components_kept"] == 1 and r["stats"]["components_dropped"] == 1
    D2 = 40.0 ** 2 + 30.0 ** 2
    assert r["D2"] == D2 and r["stats"]["zero_area_triangles"] == 0
    kept_area = sum(q for q, s in zip(r["q"], r["split_final"]) if s) * D2 / mt.FIX
    quantum = 0.5 * len(r["q"]) * D2 / mt.FIX                                    # half a unit per triangle
    assert abs(kept_area - (40.0 - 13.8) * 30.0) < quantum + 30.0 * 4e-6         # (+ the float32 rounding of the cut's x over its length)
    assert abs(r["stats"]["q_total"] * D2 / mt.FIX - 1200.0) < quantum + 30.0 * 4e-6


def covered(r, centre, radius=1.5):
    """output faces whose centroid lies within `radius` of `centre` in x, y"""
    c = r["vertices"][r["faces"]].mean(1)
    return int(((c[:, 0] - centre[0]) ** 2 + (c[:, 1] - centre[1]) ** 2 < radius ** 2).sum())


def test_islands_move_across_the_cut_by_their_area():
    V, F, val, names, r = mt.island_result(0.01)
    st = r["stats"]
    # kept side: the plane's kept region, the small high disc, the high sphere; dropped side: the strip, the two low discs, the low sphere
    assert (st["components_kept"], st["components_dropped"]) == (3, 4)
    assert (st["moved_to_kept"], st["moved_to_dropped"]) == (1, 1)
    total = st["q_total"]
    share = {c: q / total for c, q in r["Q"].items()}
    side = {c: int(r["split_side"][c]) for c in r["Q"]}
    shares = sorted((round(100 * s, 2), side[c]) for c, s in share.items())
    print("component shares of the area in % (share, side):", shares)
    small = [c for c in share if share[c] < 0.01]
    assert sorted(side[c] for c in small) == [0, 0, 1, 1]                       # a disc and a sphere on each side
    assert all(0.002 < share[c] < 0.008 for c in small)
    big = [c for c in share if 0.03 < share[c] < 0.07]
    assert len(big) == 1 and side[big[0]] == 0                                  # the 5 % hole
    for c, s in share.items():                                                  # nothing near the threshold: a last-bit difference cannot decide
        assert abs(s / 0.01 - 1.0) > 0.01
    assert covered(r, names["small_low_disc"]) > 0                              # filled back
    assert covered(r, names["big_low_disc"]) == 0                               # stays a hole
    assert covered(r, names["small_high_disc"]) == 0                            # goes
    assert covered(r, names["high_sphere"], 2.5) == 64                          # touches no cut: stays, small as it is
    assert covered(r, names["low_sphere"], 2.5) == 0


def test_without_the_island_rule_every_piece_stays_on_its_side():
    V, F, val, names, r = mt.island_result(0.0)
    st = r["stats"]
    assert (st["components_kept"], st["components_dropped"], st["moved_to_kept"], st["moved_to_dropped"]) == (3, 4, 0, 0)
    assert np.array_equal(r["split_final"], r["split_side"])
    assert covered(r, names["small_low_disc"]) == 0 and covered(r, names["big_low_disc"]) == 0
    assert covered(r, names["small_high_disc"]) > 0 and covered(r, names["high_sphere"], 2.5) == 64 and covered(r, names["low_sphere"], 2.5) == 0


def test_density_counts_and_value_by_hand():
    # eight samples at the corners of a cube: the box is the cube (scale 1), kernel depth 3 -> hk = 1/8 of the side; every sample sits on the
    # outer corner of a corner node's cell, 1/2 hk from that node: weight 1/8 to it, the other seven corners fall outside
    s = np.float32([[x, y, z] for z in (0, 8) for y in (0, 8) for x in (0, 8)])
    pts = np.float32([[0.5, 0.5, 0.5], [4, 4, 4], [0, 0, 0], [100, 0, 0], [8, 8, 8]])
    rho, value, counts = mt.density(s, None, pts, depth=5, scale=1.0, kernel_depth=3, samples_per_node=2.0)
    assert counts == (8, 0)
    assert rho.tolist() == [0.125, 0.0, 0.125 / 8, 0.0, 0.125 / 8]
    assert value[0] == 3.0 + 0.5 * math.log2(0.125 / 2.0) == 1.0 and value[1] == 0.0 and value[3] == 0.0
    assert value[2] == max(0.0, 3.0 + 0.5 * math.log2(0.125 / 16.0)) == 0.0
    # a zero normal and a NaN point are no samples; without normals only the NaN is none
    nrm = np.zeros((8, 4), np.float32)
    nrm[:, 2] = 1.0
    nrm[3, :3] = 0.0
    s2 = s.copy()
    s2[5, 1] = np.nan
    assert mt.density(s2, nrm, pts, 5, 1.0, 3)[2] == (6, 2) and mt.density(s2, None, pts, 5, 1.0, 3)[2] == (7, 1)
    # no valid sample: every value is 0
    rho, value, counts = mt.density(np.full((3, 3), np.nan, np.float32), None, pts, 5)
    assert counts == (0, 3) and not rho.any() and not value.any()
    assert mt.resolve_kernel_depth(9) == 7 and mt.resolve_kernel_depth(9, 4) == 4
