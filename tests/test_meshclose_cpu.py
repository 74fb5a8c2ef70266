"""Known answers for the numpy restatement of the hole closing (tests/meshclose_restatement.py), worked by hand, by brute force
over all triangulations or by plain counting -- the GPU tests (tests/test_gpu_meshclose.py) hold the kernels to this restatement, these hold
the restatement itself.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meshclose_restatement as mc


def test_binding_lists_the_hole_closing_and_mirrors_its_struct(tmp_path):
    from reconstruction_amd import _lib
    for name in ("rsm_mesh_close_holes", "rsm_mesh_close_holes_device", "rsm_mesh_close_holes_last", "rsm_stage_mesh_border_loops", "rsm_stage_hole_triangulate"):
        assert name in _lib.PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in _lib.MeshCloseParams._fields_]
    body = 'printf("%zu\\n", sizeof(rsm_mesh_close_params));\n' + "".join('printf("%%zu\\n", offsetof(rsm_mesh_close_params, %s));\n' % f for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsm.h"\nint main(void) {\n%sprintf("%%d\\n%%d\\n", RSM_MESH_CLOSE_MAX_HOLE, RSM_MESH_CLOSE_STATS);\n'
                   'return 0; }\n' % body)
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(root, "include"), str(src), "-o", str(tmp_path / "layout")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(_lib.MeshCloseParams) and got[-1] == _lib.MESH_CLOSE_STATS == len(mc.STAT_KEYS) and got[-2] == _lib.MESH_CLOSE_MAX_HOLE
    assert got[1:-2] == [getattr(_lib.MeshCloseParams, f).offset for f in fields]
    from reconstruction_amd._mesh import MeshPart
    assert MeshPart._CLOSE_KEYS == mc.STAT_KEYS


# ---- rings and labels by hand ---------------------------------------------------------------------------------------------------------------
def test_tetrahedron_with_two_faces_off():
    # faces (1, 2, 0) and (3, 1, 0) share the edge (0, 1): entries 2 (0 -> 1) and 4 (1 -> 0) are no border.  Border: 0 (1 -> 2), 1 (2 -> 0),
    # 3 (3 -> 1), 5 (0 -> 3).  From e0 = 0: r0 = head = 2, r1 = tail = 1, then the entry that reaches 1 is 3 (tail 3), the one that reaches 3
    # is 5 (tail 0): ring 2, 1, 3, 0.  Diagonal (r1, r3) = (1, 0) is the surviving edge: forbidden; (r0, r2) = (2, 3) remains.
    v = mc.TETRA_V
    f = np.int32([[1, 2, 0], [3, 1, 0]])
    b = mc.border_loops(f, 4)
    assert b["label"].tolist() == [0, 0, -1, 0, -1, 0] and b["size"].tolist() == [4, 4, -1, 4, -1, 4]
    assert b["loops"] == {0: [2, 1, 3, 0]} and b["open"] == []
    vo, fo, st, info = mc.close_holes(v, f)
    assert vo.tobytes() == v.tobytes() and fo.tolist() == [[1, 2, 0], [3, 1, 0], [2, 3, 0], [2, 1, 3]]
    d = mc.directed_counts(fo)
    assert len(d) == 12 and all(c == 1 and d[(b_, a)] == 1 for (a, b_), c in d.items())      # closed: every directed edge met once by its reverse
    assert (st["loops"], st["loops_closed"], st["faces_added"], st["longest_closed"], st["border_entries"]) == (1, 1, 2, 4, 4)
    # without the forbidden diagonal the areas decide: (2, 1, 0) + (1, 3, 0) = 1/2 + 1/2 against (2, 3, 0) + (2, 1, 3) = 1/2 + sqrt(3)/2
    w, tris = mc.triangulate(v[[2, 1, 3, 0]])
    assert w == 1.0 and tris.tolist() == [[0, 1, 3], [1, 2, 3]]
    F = np.zeros((4, 4), bool)
    F[1, 3] = True
    w, tris = mc.triangulate(v[[2, 1, 3, 0]], F)
    assert tris.tolist() == [[0, 2, 3], [0, 1, 2]] and abs(w - (0.5 + 0.75 ** 0.5)) < 1e-15


def test_lone_triangle_and_faces_oriented_against_each_other():
    v = mc.TETRA_V
    one = np.int32([[0, 1, 2]])
    b = mc.border_loops(one, 3)
    assert b["label"].tolist() == [0, 0, 0] and b["size"].tolist() == [3, 3, 3] and b["loops"] == {0: [1, 0, 2]}
    vo, fo, st, _ = mc.close_holes(v[:3], one)
    assert fo.tolist() == one.tolist() and (st["loops"], st["lone_triangles"], st["loops_closed"], st["longest_loop"]) == (1, 1, 0, 3)
    # (0, 1, 2) and (0, 1, 3) both hold 0 -> 1: the edge has two faces and is no border; vertex 1 has two border entries out and none in, vertex 0
    # two in and none out.  Entries 1 (1 -> 2), 2 (2 -> 0) are linked through the simple vertex 2, entries 4, 5 through 3: two open components
    against = np.int32([[0, 1, 2], [0, 1, 3]])
    b = mc.border_loops(against, 4)
    assert b["label"].tolist() == [-1, 1, 1, -1, 4, 4] and b["size"].tolist() == [-1, 0, 0, -1, 0, 0] and b["open"] == [1, 4] and b["loops"] == {}
    st = mc.close_holes(v, against)[2]
    assert (st["components"], st["open_components"], st["loops"], st["faces_added"]) == (2, 2, 0, 0)
    # oriented alike, (0, 1, 2) and (1, 0, 3) are a quad with one loop of 4: too short to be skipped, and its fill would double the two faces'
    # shared edge -- that diagonal is forbidden, the other one closes the quad into a tetrahedron
    alike = np.int32([[0, 1, 2], [1, 0, 3]])
    vo, fo, st, _ = mc.close_holes(v, alike)
    assert mc.border_loops(alike, 4)["loops"] == {1: [2, 1, 3, 0]} and fo[2:].tolist() == [[2, 3, 0], [2, 1, 3]]
    # a face with a repeated index is in no table; an empty mesh stays empty
    assert mc.border_loops(np.int32([[0, 1, 1]]), 2)["label"].tolist() == [-1, -1, -1]
    assert mc.close_holes(np.zeros((0, 3)), np.zeros((0, 3)))[1].shape == (0, 3) and mc.close_holes(v, np.zeros((0, 3)))[2]["n_faces"] == 0


def test_the_cut_plane_has_its_four_loops_and_a_bow_tie_has_none():
    v, f = mc.cut_plane()
    b = mc.border_loops(f, len(v))
    assert sorted(len(r) for r in b["loops"].values()) == [3, 4, 6, 32] and b["open"] == [] and b["n_border"] == 45
    assert len(b["loops"][0]) == 32                                               # the outer border holds the lowest entry
    assert 6 * 9 + 4 not in f                                                     # the fan's centre is unreferenced
    # two removed cells that share a corner: four border entries at that vertex, which is not simple -- both holes are open
    pv, pf = mc.plane(5, 5)
    cells = 16
    bow = mc.remove_faces(pf, [1 * 4 + 1, cells + 1 * 4 + 1, 2 * 4 + 2, cells + 2 * 4 + 2])
    b = mc.border_loops(bow, len(pv))
    assert len(b["components"]) == 3 and len(b["open"]) == 2 and [len(r) for r in b["loops"].values()] == [16]
    assert sorted(len(b["components"][c]) for c in b["open"]) == [4, 4]
    st = mc.close_holes(pv, bow, 30)[2]
    assert (st["open_components"], st["loops"], st["loops_closed"], st["faces_added"]) == (2, 1, 1, 14)   # (the outer border is a loop of 16: it is closed too)
    assert mc.close_holes(pv, bow, 15)[2]["faces_added"] == 0


# ---- rule 7 against brute force ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 4, 5, 6, 7, 8, 9])
def test_triangulation_is_the_least_over_all_triangulations(L):
    catalan = [1, 1, 2, 5, 14, 42, 132, 429]
    for seed in range(3):
        p = mc.ring_points(L, seed)
        w, tris = mc.triangulate(p)
        best, count = mc.brute_force(p)
        assert count == catalan[L - 2] == len(mc.all_triangulations(0, L - 1))
        assert abs(w - best) <= 4 * L * np.spacing(best) and len(tris) == L - 2
        P = mc._points(p)
        assert abs(sum(mc.tri_area(P[i], P[k], P[j]) for i, k, j in tris.tolist()) - w) <= 4 * L * np.spacing(w)
        if L >= 4:                                                                 # forbid a diagonal the free optimum uses
            i, k, j = next(t for t in tris.tolist() if max(t[1] - t[0], t[2] - t[1]) >= 2)
            F = np.zeros((L, L), bool)
            F[(i, k) if k - i >= 2 else (k, j)] = True
            w2, tris2 = mc.triangulate(p, F)
            best2, count2 = mc.brute_force(p, F)
            assert count2 < count and (w2 == best2 == mc.INF if count2 == 0 else abs(w2 - best2) <= 4 * L * np.spacing(best2)) and w2 >= w
            used = {(a, b) for t in tris2.tolist() for a, b in ((t[0], t[1]), (t[1], t[2]), (t[0], t[2]))}
            assert not any(F[a, b] for a, b in used)


def test_ties_go_to_the_lowest_k_and_collinear_points_make_no_zero_area_face():
    # the unit square: both diagonals cost 1/2 + 1/2; k = 1 comes first
    sq = np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    w, tris = mc.triangulate(sq)
    assert w == 1.0 and tris.tolist() == [[0, 1, 3], [1, 2, 3]]
    # a 2 x 2 square with the midpoint of its first side: (0, 1, 2) is without area and never used, though it would be the cheapest ear
    ring = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]])
    w, tris = mc.triangulate(ring)
    P = mc._points(ring)
    assert w == 4.0 and all(mc.tri_n2(P[i], P[k], P[j]) > 0.0 for i, k, j in tris.tolist()) and [0, 1, 2] not in tris.tolist()
    assert abs(mc.brute_force(ring)[0] - 4.0) < 1e-15 and mc.brute_force(ring)[1] == 3        # of 5
    # three collinear points, or every diagonal forbidden: no triangulation
    assert mc.triangulate(ring[:3])[0] == mc.INF and mc.triangulate(ring[:3])[1].shape == (0, 3)
    F = np.ones((4, 4), bool)
    assert mc.triangulate(sq, F)[0] == mc.INF and mc.brute_force(sq, F) == (mc.INF, 0)
    v, f = mc.collinear_hole()
    st = mc.close_holes(v, f, 8)[2]                                                # (the outer border has 16 edges)
    assert (st["loops_untriangulated"], st["loops_closed"], st["loops_too_long"], st["faces_added"]) == (1, 0, 1, 0)


# ---- the post-conditions by plain counting -----------------------------------------------------------------------------------------------------
def test_post_conditions_on_the_scenes():
    v, f = mc.cut_plane()
    vo, fo, st, info = mc.close_holes(v, f, 30)
    assert mc.check_closed(v, f, fo, info) == 3 + 4 + 6 and st["faces_added"] == 1 + 2 + 4 and st["loops_too_long"] == 1
    v, f, holes = mc.many_holes()
    vo, fo, st, info = mc.close_holes(v, f, 30)
    assert holes > 256 and st["loops_closed"] == holes and mc.check_closed(v, f, fo, info) == st["border_entries"] - 140
    assert list(info["closed"]) == sorted(info["closed"])                          # ascending label
    for L, m, closed in ((30, 30, 1), (31, 30, 0), (64, 64, 1)):
        v, f = mc.annulus(L)
        vo, fo, st, info = mc.close_holes(v, f, m)
        assert st["loops"] == 2 and st["loops_closed"] == closed and st["faces_added"] == closed * (L - 2) and st["longest_loop"] == 2 * L
        mc.check_closed(v, f, fo, info)
    # the whole tetrahedron has no border, and closing is idempotent
    st = mc.close_holes(mc.TETRA_V, mc.TETRA_F)[2]
    assert st["border_entries"] == 0 and st["components"] == 0
    v, f = mc.cut_plane()
    _, fo, _, _ = mc.close_holes(v, f, 32)
    assert mc.close_holes(v, fo, 32)[2]["faces_added"] == 0 and mc.close_holes(v, fo, 32)[2]["border_entries"] == 0
