"""The numpy restatement of the mesh decimation (tests/meshdecimate_restatement.py) held to known answers and invariants on the
CPU; tests/test_gpu_meshdecimate.py holds the kernels to the restatement byte for byte.  Nothing here reads the restatement's own tables to
check its results: edge counts, adjacency, areas and normals are recomputed from the face lists."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import meshdecimate_restatement as md

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rsm.h")


def face_normals(V, F):
    P = np.asarray(V, np.float64)
    return np.cross(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]])


def area(V, F):
    return 0.5 * np.linalg.norm(face_normals(V, F), axis=1).sum()


def neighbours(F, nv):
    nb = [set() for _ in range(nv)]
    for a, b, c in np.asarray(F).tolist():
        nb[a] |= {b, c}
        nb[b] |= {a, c}
        nb[c] |= {a, b}
    return nb


@pytest.fixture(scope="module")
def whole():
    """every whole-call case of the GPU tests, decimated once"""
    return {name: (mesh, p) + md.decimate(mesh[0], mesh[1], p) for name, mesh, p in md.whole_cases()}


# ---- known answers --------------------------------------------------------------------------------------------------------------------------
def test_lone_triangle_quadrics_by_hand():
    V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    F = np.int32([[0, 1, 2]])
    for bw in (1.0, 2.0):
        w = bw * bw
        Q = md.quadrics(V, F, bw)
        # face: the plane z = 0 with n = (0, 0, 1): zz = 1.  Borders: (0,1) -> y = 0, (2,0) -> x = 0, (1,2) -> (x + y - 1) / sqrt 2 = 0
        want0 = [w, 0, 0, 0, w, 0, 0, 1, 0, 0]
        want1 = [0.5 * w, 0.5 * w, 0, -0.5 * w, 1.5 * w, 0, -0.5 * w, 1, 0, 0.5 * w]
        want2 = [1.5 * w, 0.5 * w, 0, -0.5 * w, 0.5 * w, 0, -0.5 * w, 1, 0, 0.5 * w]
        assert np.allclose(Q, [want0, want1, want2], rtol=0, atol=4e-16 * w)
    # not normalised: a triangle of twice the area weighs four times (n = (0, 0, 2))
    V2 = np.float32([[0, 0, 0], [2, 0, 0], [0, 1, 0], [5, 5, 5]])
    Q2 = md.quadrics(V2, F)
    assert Q2[0, 7] == 4.0 and (Q2[3] == 0).all()


def test_border_plane_by_hand_for_both_weights():
    """one border edge of a tilted face: the plane through the edge perpendicular to the face, |m| = boundary_weight |n|"""
    V = np.float32([[1, 1, 1], [3, 1, 1], [1, 1, 4]])                             # a face in the plane y = 1, n = (0, -6, 0)
    n = np.array([[0.0, -6.0, 0.0]])
    Pa, Pb = V[[0]].astype(np.float64), V[[1]].astype(np.float64)                  # the edge along x at z = 1: its border plane is z = 1
    for bw in (1.0, 2.0):
        q, has = md._border_quadric(n, Pa, Pb, bw)
        m = 6.0 * bw                                                               # n x e / |e| = (0, -6, 0) x (1, 0, 0) = (0, 0, 6)
        assert has[0] and np.array_equal(q[0], [0, 0, 0, 0, 0, 0, 0, m * m, -m * m, m * m])
        assert md._qerr(q, np.array([[7.0, -3.0, 1.0]]))[0] == 0.0 and md._qerr(q, np.array([[0.0, 0.0, 3.0]]))[0] == (2 * m) ** 2
    q, has = md._border_quadric(n, Pa, Pa, 1.0)                                    # an edge without length adds nothing
    assert not has[0] and (q == 0).all()
    Q1, Q2 = md.quadrics(V, np.int32([[0, 1, 2]]), 1.0), md.quadrics(V, np.int32([[0, 1, 2]]), 2.0)
    Kf = md._plane_quadric(n, np.array([6.0]))
    assert np.allclose(Q2 - Kf, 4.0 * (Q1 - Kf), rtol=1e-15, atol=0)


def test_the_optimum_of_an_edge_at_a_corner_is_the_corner():
    V, F = md.corner_mesh()
    Q = md.quadrics(V, F)
    corner = V[0].astype(np.float64)
    for b in (1, 2, 3):                                                            # the edges along the axes: their other end is no border vertex
        Qe = (Q[0] + Q[b])[None]
        pos, branch = md.placement(Qe, V[[0]].astype(np.float64), V[[b]].astype(np.float64), 1)
        assert branch[0] == md.B_OPTIMAL and np.array_equal(pos[0], V[0])
        assert abs(md._qerr(Qe, corner[None])[0]) <= 1e-12 * Qe[0, 9]
    key, mult, cost, reject, pos, _ = md.collapse_costs(V, F, Q, md.params())
    at_corner = [e for e in range(len(key)) if int(key[e]) >> 32 == 0 and int(key[e]) & 0xFFFFFFFF in (1, 2, 3)]
    assert len(at_corner) == 3
    for e in at_corner:
        assert reject[e] == 0 and np.array_equal(pos[e], V[0]) and cost[e] == 1e-15 / 0.3


def test_placement_branches():
    one = lambda q: np.array([q], np.float64)
    Pa, Pb = one([0.0, 0, 0]), one([1.0, 0, 0])
    flat = one([0, 0, 0, 0, 0, 0, 0, 1, 0, 0])                                     # the plane z = 0: singular, every point of the edge at error 0
    assert md.placement(flat, Pa, Pb, 1)[1][0] == md.B_PA                          # ties go Pa, Pb, mid
    px = lambda c: one([1, 0, 0, -c, 1, 0, 0, 1, 0, c * c])                        # (x - c)^2 + y^2 + z^2
    assert md.placement(px(0.25), Pa, Pb, 1) [1][0] == md.B_OPTIMAL and md.placement(px(0.25), Pa, Pb, 1)[0][0, 0] == 0.25
    assert md.placement(px(2.5), Pa, Pb, 1)[1][0] == md.B_OPTIMAL                  # |x - mid| = 2 = 2 |e|: still inside the guard
    assert md.placement(px(2.75), Pa, Pb, 1)[1][0] == md.B_PB                      # beyond it: the best of the three
    assert md.placement(px(0.25), Pa, Pb, 0)[1][0] == md.B_PA and md.placement(px(0.5), Pa, Pb, 0)[1][0] == md.B_MID
    assert md.placement(px(0.9), Pa, Pb, 0)[1][0] == md.B_PB


# ---- invariants -------------------------------------------------------------------------------------------------------------------------------
def test_tetrahedron_has_no_candidate():
    V, F = md.TETRA
    key, mult, cost, reject, pos, _ = md.collapse_costs(V, F, md.quadrics(V, F), md.params())
    assert len(key) == 6 and (mult == 2).all() and np.isinf(cost).all() and (reject == md.R_DUPLICATE).all()
    Vo, Fo, st = md.decimate(V, F, md.params(target_faces=2))
    assert np.array_equal(Fo, F) and st["rounds"] == 1 and st["collapses"] == 0 and st["target_reached"] == 0 and st["rejected_duplicate"] == 6
    # without the topology rules the duplicate rule still holds it
    assert (md.collapse_costs(V, F, md.quadrics(V, F), md.params(preserve_topology=0))[3] == md.R_DUPLICATE).all()


def test_octahedron_link_rule_and_target_6():
    """Every edge of the octahedron has exactly its two opposite vertices as common neighbours: the link rule rejects none of the twelve, all
    cost the same, and the lowest key (0, 2) collapses: 8 -> 6 faces, the double pyramid over a triangle.  Of its nine edges the link rule
    rejects the three of the middle triangle: their ends share both apexes and the third vertex of the triangle, three for two faces."""
    V, F = md.OCTA
    key, mult, cost, reject, pos, _ = md.collapse_costs(V, F, md.quadrics(V, F), md.params())
    assert len(key) == 12 and (reject == 0).all() and len(set(cost.tolist())) == 1
    Vo, Fo, st = md.decimate(V, F, md.params(target_faces=6))
    assert len(Fo) == 6 and len(Vo) == 5 and st["collapses"] == 1 and st["rounds"] == 1 and st["target_reached"] == 1
    r = md.collapse_round(V, F, md.quadrics(V, F), 2, md.params())
    assert r["selected"].tolist() == [(0 << 32) | 2] and r["kept"] == 1
    # the double pyramid over a triangle that is left: its three base edges fail the link rule (the two apexes and the third base vertex)
    k2, m2, c2, r2, _, _ = md.collapse_costs(Vo, Fo, md.quadrics(Vo, Fo), md.params())
    nb = neighbours(Fo, len(Vo))
    want = [md.R_LINK if len(nb[int(k) >> 32] & nb[int(k) & 0xFFFFFFFF]) != 2 else 0 for k in k2]
    assert len(k2) == 9 and (r2 & 15).tolist() == want and want.count(md.R_LINK) == 3


def test_three_face_edge_locks_its_endpoints():
    V, F = md.FAN3
    key, mult, cost, reject, pos, T = md.collapse_costs(V, F, md.quadrics(V, F), md.params())
    by = {(int(k) >> 32, int(k) & 0xFFFFFFFF): (int(m), int(r)) for k, m, r in zip(key, mult, reject)}
    assert by[(0, 1)] == (3, md.R_NONMANIFOLD) and T.locked.tolist() == [True, True, False, False, False, False]
    for (a, b), (m, r) in by.items():
        if (a, b) != (0, 1):
            assert (r & 15 == md.R_LOCKED) == (a in (0, 1) or b in (0, 1)), (a, b, r)
    assert by[(2, 5)][1] & 15 == 0


def test_border_rules():
    V, F = md.grid_mesh(5)
    key, mult, cost, reject, pos, T = md.collapse_costs(V, F, md.quadrics(V, F), md.params())
    k, c = md.edge_counts(F)
    border_v = set((k[c == 1] >> 32).tolist()) | set((k[c == 1] & 0xFFFFFFFF).tolist())
    for kk, m, r in zip(key.tolist(), mult.tolist(), reject.tolist()):
        a, b = kk >> 32, kk & 0xFFFFFFFF
        if a in border_v and b in border_v and m == 2:
            assert r & 15 == md.R_BORDER                                            # a chord between two border vertices would pinch the mesh
    assert (reject & 15 == md.R_BORDER).sum() == 2                                 # the diagonals of the two corner cells cut from border to border
    locked = md.collapse_costs(V, F, md.quadrics(V, F), md.params(preserve_boundary=1))[3]
    for kk, r in zip(key.tolist(), locked.tolist()):
        assert (r & 15 == md.R_LOCKED) == ((kk >> 32) in border_v or (kk & 0xFFFFFFFF) in border_v)


def test_a_rounds_selection_is_independent_and_the_scan_cuts_it():
    V, F = md.grid_mesh(21, md.bumpy)
    Q = md.quadrics(V, F)
    nb = neighbours(F, len(V))
    r = md.collapse_round(V, F, Q, 300, md.params())
    sel = [(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in r["selected"]]
    assert len(sel) >= 10
    for i, (a, b) in enumerate(sel):
        for c, d in sel[i + 1:]:
            assert not ({a, b} & {c, d}) and not (nb[a] | nb[b]) & {c, d}, ((a, b), (c, d))
    # the global minimum is always selected
    key, mult, cost, reject, _, _ = md.collapse_costs(V, F, Q, md.params())
    assert int(r["selected"][0]) == int(key[np.argsort(cost, kind="stable")[0]])
    # kept while the faces removed before are fewer than need
    k, c = md.edge_counts(F)
    m = [int(c[np.searchsorted(k, (a << 32) | b)]) for a, b in sel]
    for need in (1, 2, 3, 7):
        rn = md.collapse_round(V, F, Q, need, md.params())
        sn = [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in rn["selected"]]
        mn = [int(c[np.searchsorted(k, (a << 32) | b)]) for a, b in sn]
        kept = sum(1 for i in range(len(sn)) if sum(mn[:i]) < need)
        total = sum(mn[:kept])
        assert rn["kept"] == kept >= 1 and len(F) - len(rn["F"]) == total
        assert need <= total <= need + 1 or kept == len(sn)                        # need or one more, unless the selection ran out first


# ---- whole meshes -----------------------------------------------------------------------------------------------------------------------------
def test_flat_plane_with_its_boundary_kept():
    V, F = md.grid_mesh(21, None, 0.3)
    Vo, Fo, st = md.decimate(V, F, md.params(target_faces=200, preserve_boundary=1))
    assert len(Fo) in (199, 200) and st["target_reached"] == 1
    assert (Vo[:, 2] == 0).all()
    assert abs(area(Vo, Fo) - 400.0) <= 1e-9 * 400.0
    assert (face_normals(Vo, Fo)[:, 2] > 0).all()
    # the boundary's vertices are all there
    edge = lambda A: set(map(tuple, A[(A[:, 0] == 0) | (A[:, 0] == 20) | (A[:, 1] == 0) | (A[:, 1] == 20)].tolist()))
    assert edge(Vo) == edge(V) and len(edge(V)) == 80 and st["locked_vertices"] == 80


def test_icosphere_stays_a_sphere(whole):
    (V, F), p, Vo, Fo, st = whole["icosphere_320"]
    assert len(F) == 1280 and len(Fo) in (319, 320)
    k, c = md.edge_counts(Fo)
    assert (c == 2).all() and len(Vo) - len(k) + len(Fo) == 2
    assert st["border_collapses"] == 0 and st["collapses"] == len(V) - len(Vo)


def test_height_field_ends_at_the_target_with_one_border_loop(whole):
    (V, F), p, Vo, Fo, st = whole["height_field_160"]
    assert len(F) == 800 and len(Fo) in (159, 160) and st["target_reached"] == 1 and 5 <= st["rounds"] <= 60
    k, c = md.edge_counts(Fo)
    assert c.max() == 2 and md.border_loops(Fo) == 1 and st["border_collapses"] > 0
    assert len(Vo) - len(k) + len(Fo) == 1                                         # still a disc


def test_preserve_normal_keeps_every_face_up(whole):
    (V, F), p, Vo, Fo, st = whole["height_field_normals"]
    assert p["preserve_normal"] == 1 and (face_normals(Vo, Fo)[:, 2] > 0).all()
    V2, F2, st2 = md.decimate(V, F, md.params(target_faces=160, preserve_normal=1))
    assert (face_normals(V2, F2)[:, 2] > 0).all() and len(F2) in (159, 160)


def test_every_whole_case_of_the_gpu_tests_ends_at_target_or_one_below(whole):
    for name, ((V, F), p, Vo, Fo, st) in whole.items():
        t = md.resolve_target(p, len(F))
        assert len(Fo) in (t - 1, t) and st["target"] == t and st["target_reached"] == 1, (name, len(Fo), t)
        assert st["n_faces"] == len(Fo) and st["n_vertices"] == len(Vo) and Fo.max() == len(Vo) - 1
        assert st["rounds"] <= 60, (name, st["rounds"])
    assert md.resolve_target(md.params(target_fraction=0.2), 800) == 160 and md.resolve_target(md.params(target_faces=7, target_fraction=1.0), 9) == 9


def test_autoclean_repeated_indices_and_targets_at_the_ends():
    V, F = md.grid_mesh(5)
    V2 = np.concatenate([V[:3], np.float32([[9, 9, 9]]), V[3:]])                    # an unreferenced vertex in the middle
    F2 = np.where(F >= 3, F + 1, F).astype(np.int32)
    F2 = np.concatenate([F2[:4], np.int32([[0, 0, 1], [5, 5, 5]]), F2[4:]])
    Vo, Fo, st = md.decimate(V2, F2, md.params(target_faces=1000))
    assert st["rounds"] == 0 and st["repeated_index_faces"] == 2 and np.array_equal(Vo, V) and np.array_equal(Fo, F) and st["target_reached"] == 1
    Vz, Fz, sz = md.decimate(V, F, md.params(target_faces=0))
    assert sz["target_reached"] == int(len(Fz) == 0) and sz["collapses"] > 0 and (md.edge_counts(Fz)[1].max() <= 2 if len(Fz) else True)
    e3, e3i = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    Ve, Fe, se = md.decimate(e3, e3i, md.params())
    assert Ve.shape == (0, 3) and Fe.shape == (0, 3) and se["target_reached"] == 1
    Vn, Fn, sn = md.decimate(V, e3i, md.params())
    assert Vn.shape == (0, 3) and Fn.shape == (0, 3)
    # max_rounds = 1 is the round stage
    hv, hf = md.grid_mesh(21, md.bumpy)
    p = md.params(target_faces=160, max_rounds=1)
    V1, F1, s1 = md.decimate(hv, hf, p)
    r = md.collapse_round(hv, hf, md.quadrics(hv, hf), 640, p)
    used = np.zeros(len(hv), bool)
    used[r["F"].ravel()] = True
    assert np.array_equal(V1, r["V"][used]) and len(F1) == len(r["F"]) and s1["rounds"] == 1 and s1["collapses"] == r["kept"] and s1["target_reached"] == 0


# ---- the binding's mirror of the parameters, as the C compiler sees the struct -----------------------------------------------------------------
def test_params_struct_layout_and_stats_count(tmp_path):
    from reconstruction_amd import _lib
    c = _lib.MeshDecimateParams
    src = tmp_path / "layout.c"
    body = 'printf("size %zu\\n", sizeof(rsm_mesh_decimate_params));\n' + "".join(
        'printf("%s %%zu\\n", offsetof(rsm_mesh_decimate_params, %s));\n' % (f, f) for f, _ in c._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsm.h"\nint main(void) {\n%sprintf("stats %%d\\n", RSM_MESH_DECIMATE_STATS);\nreturn 0; }\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(c)
    for f, _ in c._fields_:
        assert int(got[f]) == getattr(c, f).offset, f
    assert int(got["stats"]) == _lib.MESH_DECIMATE_STATS == len(md.STAT_KEYS)
    from reconstruction_amd._mesh import MeshPart
    assert MeshPart._DECIMATE_KEYS == md.STAT_KEYS
    for name in ("rsm_mesh_decimate", "rsm_mesh_decimate_device", "rsm_mesh_decimate_last", "rsm_stage_mesh_quadrics", "rsm_stage_mesh_collapse_costs",
                 "rsm_stage_mesh_collapse_round"):
        assert name in _lib.PROTOTYPES and re.search(r"\b%s\s*\(" % name, open(HEADER).read())
