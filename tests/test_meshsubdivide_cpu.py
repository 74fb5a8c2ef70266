"""tests/meshsubdivide_restatement.py -- which tests/test_gpu_meshsubdivide.py holds the GPU Loop subdivision to, byte for byte -- held to
things it does not compute itself: Euler's formula and orientation on closed solids, the exact arithmetic of a regular integer lattice, the
1/8 3/4 1/8 border rule, the convex hull, conformity of adaptive runs, and the coverage of its own pattern fixtures; and csrc/subdivide_limits.h
against 128-bit arithmetic (tests/cpp/subdivide_limits_check.cpp, plain g++).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import mesh_topology_fixtures as mt
import meshsubdivide_restatement as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLIDS = {"tetrahedron": ms.tetrahedron, "octahedron": ms.octahedron, "icosahedron": ms.icosahedron}


def directed(F):
    d = {}
    for a, b, c in F.tolist():
        for e in ((a, b), (b, c), (c, a)):
            d[e] = d.get(e, 0) + 1
    return d


def euler(nv, F):
    d = directed(F)
    return nv - len({(min(e), max(e)) for e in d}) + len(F)


@pytest.mark.parametrize("name", sorted(SOLIDS))
def test_closed_solids_keep_their_topology_over_three_iterations(name):
    v, f = SOLIDS[name]()
    assert euler(len(v), f) == 2
    for _ in range(3):
        ne = len(ms.edge_runs(f))
        w = ms.loop_step(v, f, 0.0)
        assert len(w["V"]) == len(v) + ne and len(w["F"]) == 4 * len(f)
        d = directed(w["F"])
        assert all(n == 1 for n in d.values()) and all((b, a) in d for a, b in d)      # every directed edge once, and its reverse once
        assert euler(len(w["V"]), w["F"]) == 2
        assert (w["vertex_class"] == ms.V_INTERIOR).all() and w["patterns"] == [0, 0, 0, len(f)]
        v, f = w["V"], w["F"]
    sv, sf, st = ms.subdivide(*SOLIDS[name](), iterations=3)
    assert sv.tobytes() == v.tobytes() and sf.tobytes() == f.tobytes() and st["iterations"] == 3 and st["n_faces"] == 64 * st["n_faces_in"]


@pytest.mark.parametrize("name", sorted(SOLIDS))
def test_convex_solids_stay_inside_their_hull(name):
    v, f = SOLIDS[name]()
    r = np.linalg.norm(v.astype(np.float64), axis=1).max()
    for it in (1, 2, 3):
        ov, _, _ = ms.subdivide(v, f, iterations=it)
        assert np.linalg.norm(ov.astype(np.float64), axis=1).max() <= r * (1.0 + 2.0 ** -22)


def test_beta_is_loops():
    assert abs(ms.beta(3) - 3.0 / 16.0) < 1e-15 and abs(ms.beta(6) - 1.0 / 16.0) < 1e-15
    for k in range(3, 1001):
        b = ms.beta(k)
        assert 0.0 < k * b < 1.0 and abs(b - (5.0 / 8.0 - (3.0 / 8.0 + np.cos(2.0 * np.pi / k) / 4.0) ** 2) / k) < 1e-15


def test_integer_lattice_is_reproduced_exactly():
    v, f = ms.lattice()
    inner = ms.lattice_interior()
    w = ms.loop_step(v, f, 0.0)
    assert inner.sum() == 20 and (w["vertex_class"][inner] == ms.V_INTERIOR).all() and (w["vertex_class"][~inner] != ms.V_INTERIOR).all()
    assert w["even"][inner].tobytes() == v[inner].tobytes()                           # 1 - 6 beta + 6 beta of a symmetric ring: the vertex itself
    two = w["multiplicity"] == 2
    mid = np.array([(v[int(k) >> 32].astype(np.float64) + v[int(k) & 0xFFFFFFFF].astype(np.float64)) / 2 for k in w["keys"]]).astype(np.float32)
    assert two.sum() > 50 and w["odd"][two].tobytes() == mid[two].tobytes()           # 3/8 (a + b) + 1/8 (c + d) with c + d = a + b
    assert w["odd"][~two].tobytes() == mid[~two].tobytes() and w["max_valence"] == 6


def test_border_rule_corners_and_the_bow_tie():
    n = 4
    v, f = ms.square_patch(n)
    w = ms.loop_step(v, f, 0.0)
    P = v.astype(np.float64)
    idx = lambda i, j: j * n + i
    for i in range(1, n - 1):                                                          # the straight sides: 1/8 + 3/4 + 1/8 of collinear points
        for a, p, q in ((idx(i, 0), idx(i - 1, 0), idx(i + 1, 0)), (idx(0, i), idx(0, i - 1), idx(0, i + 1))):
            assert w["vertex_class"][a] == ms.V_BORDER
            assert w["even"][a].tobytes() == (P[a] * 0.75 + (P[p] + P[q]) * 0.125).astype(np.float32).tobytes() == v[a].tobytes()
    for a, p, q in ((idx(0, 0), idx(1, 0), idx(0, 1)), (idx(n - 1, 0), idx(n - 2, 0), idx(n - 1, 1)), (idx(n - 1, n - 1), idx(n - 2, n - 1), idx(n - 1, n - 2))):
        assert w["vertex_class"][a] == ms.V_BORDER                                     # a corner has two border edges: it moves inwards
        want = (P[a] * 0.75 + (P[p] + P[q]) * 0.125).astype(np.float32)
        assert w["even"][a].tobytes() == want.tobytes() and want.tobytes() != v[a].tobytes()
    assert w["moved_border"] == 4 * (n - 1) and w["moved_interior"] == (n - 2) ** 2 and w["locked"] == 0
    bv, bf = ms.bow_tie()
    b = ms.loop_step(bv, bf, 0.0)
    assert b["vertex_class"].tolist() == [1, 1, 2, 1, 1] and b["even"][2].tobytes() == bv[2].tobytes() and (b["even"][[0, 1, 3, 4]] != bv[[0, 1, 3, 4]]).any(1).all()
    tv, tf = ms.three_face_edge()
    t = ms.loop_step(tv, tf, 0.0)
    assert t["vertex_class"].tolist() == [2, 2, 1, 1, 1] and t["split_many"] == 1 and t["even"][:2].tobytes() == tv[:2].tobytes()
    assert t["odd"][0].tobytes() == ((tv[0].astype(np.float64) + tv[1].astype(np.float64)) * 0.5).astype(np.float32).tobytes()


def conforming(F_in, w):
    """every input edge is kept whole in all its faces or replaced by its two halves in all: no output edge runs past a new vertex (faces
    with a repeated index have no area and take no part in the edge table: they pass through as they are and are not looked at here)"""
    und = {(min(e), max(e)) for e in directed(w["F"][[ms.distinct(t) for t in w["F"].tolist()]])}
    for k, s, i in zip(w["keys"].tolist(), w["split"].tolist(), range(len(w["keys"]))):
        a, b = k >> 32, k & 0xFFFFFFFF
        if s:
            m = len(w["even"]) + int(w["split"][:i].sum())
            if (a, b) in und or (a, m) not in und or (b, m) not in und:
                return False
        elif (a, b) not in und:
            return False
    return True


@pytest.mark.parametrize("thr", [0.0, 0.9, 1.0, 1.1, 1.3, 1.45, 2.0])
def test_adaptive_runs_are_conforming_and_keep_orientation(thr):
    v, f = mt.grid()
    w = ms.loop_step(v, f, thr)
    assert conforming(f, w)
    assert len(w["F"]) == len(f) + sum(c * n for c, n in enumerate(w["patterns"])) and len(w["V"]) == len(v) + w["n_split"]
    d = directed(w["F"])
    assert all(n == 1 for n in d.values())                                             # the input is an oriented manifold: so is the output
    assert euler(len(w["V"]), w["F"]) == euler(len(v), f)
    # signed area in the xy plane (the grid is a jittered height field): no face is turned over
    P = w["V"].astype(np.float64)
    A, B, C3 = P[w["F"][:, 0]], P[w["F"][:, 1]], P[w["F"][:, 2]]
    assert (((B - A)[:, 0] * (C3 - A)[:, 1] - (B - A)[:, 1] * (C3 - A)[:, 0]) > 0).all()
    if thr == 2.0:
        assert w["n_split"] == 0 and w["F"].tobytes() == f.tobytes() and w["V"].tobytes() == v.tobytes()


def test_pattern_fixtures_reach_every_pattern_both_diagonals_and_the_tie():
    v, f = ms.pattern_mesh()
    w = ms.loop_step(v, f, ms.PATTERN_THR)
    assert w["patterns"] == ms.PATTERN_COUNTS == [2, 4, 6, 2]
    assert w["diagonals"] == ms.PATTERN_DIAGONALS == [1, 2, 3]
    assert conforming(f, w) and len(w["F"]) == 2 * 1 + 4 * 2 + 6 * 3 + 2 * 4
    # a threshold exactly at a length: that edge stays; the next double below: it splits
    tv, tf = np.float32([[0, 0, 0], [3, 0, 0], [3, 4, 0]]), np.int32([[0, 1, 2]])
    assert ms.loop_step(tv, tf, 5.0)["n_split"] == 0 and ms.loop_step(tv, tf, float(np.nextafter(5.0, 0.0)))["n_split"] == 1
    g = ms.loop_step(*mt.grid(), 1.1)
    assert min(g["patterns"][1:]) > 0
    ov, of, st = ms.subdivide(v, f, iterations=8, threshold=ms.PATTERN_THR)           # the call ends once nothing is longer than the threshold
    assert st["iterations"] < 8 and all(np.sqrt(ms.len2(ov[a].astype(np.float64), ov[b].astype(np.float64))) <= ms.PATTERN_THR for (a, b), _ in ms.edge_runs(of))


def test_size_limits_against_128_bit_arithmetic(tmp_path):
    exe = tmp_path / "subdivide_limits_check"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-I" + os.path.join(ROOT, "reconstruction_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "subdivide_limits_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stderr[-500:], [l for l in r.stdout.splitlines() if l.split()[3] != l.split()[4]][:5])
    rows = [tuple(int(t) for t in l.split()) for l in r.stdout.splitlines()]
    assert len(rows) >= 300 and all(row[3] == row[4] for row in rows)
    by = {(row[0] + row[1], row[2]): row[3] for row in rows}
    imax, big = 2 ** 31 - 1, 2 ** 31
    assert by[(imax, (big - 2) // 3)] == 1 and by[(imax + 1, (big - 2) // 3)] == 0 and by[(imax, (big + 1) // 3)] == 0 and by[(imax, (big - 5) // 3)] == 1
