"""Loop subdivision of a triangle mesh as DESIGN.md 9 (f15) defines it, restated with numpy, plain dicts and loops -- written from the rules,
not from csrc/k_meshsubdivide.hip, which tests/test_gpu_meshsubdivide.py holds to this file byte for byte.

One iteration (loop_step), everything in float64, float32 only where a position is stored:
  edges      the unique edges (a, b), a < b, of the faces without a repeated index, in the order of the key (a << 32) | b; a run = the entries
             3 f + j of the faces on the edge, ascending.  An edge splits when ((dx dx + dy dy) + dz dz) > thr thr; the r-th split edge in
             key order gets the new vertex nv + r
  odd        an edge in exactly two faces, c and d opposite it in the run's order: ((Pa + Pb) 0.375) + ((Pc + Pd) 0.125); else (Pa + Pb) 0.5
  classes    locked: at an edge of three or more faces, or with border edges but not exactly two, or in no face; border: exactly two border
             edges; interior: the rest
  even       only a vertex that is not locked and has an edge that splits moves.  Interior, k corners: S over the corner list, ascending,
             S = S + P[next]; S = S + P[prev]; P (1 - k beta_k) + (S 0.5) beta_k, beta_k = (0.625 - t t) / k, t = 0.375 + 0.25 cos(2 pi / k)
             with math.cos.  Border, border neighbours p, q: P 0.75 + (Pp + Pq) 0.125
  faces      in input order, each replaced by 1 + its split edges faces; the quad of the two-split pattern is cut along the shorter of its
             diagonals in the iteration's OUTPUT positions, from v_j on a tie
subdivide() runs up to `iterations` of them with one threshold and stops at the first that splits nothing."""
from __future__ import annotations

import math

import numpy as np

V_INTERIOR, V_BORDER, V_LOCKED = 0, 1, 2
STAT_KEYS = ("n_vertices_in", "n_faces_in", "n_vertices", "n_faces", "iterations", "threshold", "split_edges", "split_border_edges", "split_many_face_edges",
             "faces_0_splits", "faces_1_split", "faces_2_splits", "faces_3_splits", "moved_interior", "moved_border", "locked_vertices", "max_valence")


def beta(k):
    t = 0.375 + 0.25 * math.cos((2.0 * math.pi) / k)
    return (0.625 - t * t) / k


def _mesh(V, F):
    return np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(F, np.int32).reshape(-1, 3)


def distinct(face):
    return face[0] != face[1] and face[1] != face[2] and face[0] != face[2]


def edge_runs(F):
    """[((a, b), [entries 3 f + j, ascending])] in key order"""
    runs = {}
    for f, face in enumerate(F.tolist()):
        if not distinct(face):
            continue
        for j in range(3):
            p, q = face[j], face[(j + 1) % 3]
            runs.setdefault((min(p, q), max(p, q)), []).append(3 * f + j)
    return sorted(runs.items())


def len2(p, q):
    dx, dy, dz = float(p[0]) - float(q[0]), float(p[1]) - float(q[1]), float(p[2]) - float(q[2])
    return (dx * dx + dy * dy) + dz * dz


def box_diagonal(V):
    """the fp64 diagonal of the float32 box of all vertices (0 without a vertex)"""
    V = np.ascontiguousarray(V, np.float32).reshape(-1, 3)
    if len(V) == 0:
        return 0.0
    d = V.max(0).astype(np.float64) - V.min(0).astype(np.float64)
    return math.sqrt((float(d[0]) * float(d[0]) + float(d[1]) * float(d[1])) + float(d[2]) * float(d[2]))


def loop_step(V, F, thr):
    """one iteration -> dict: V, F (the result), keys, multiplicity, split, odd (per unique edge), vertex_class, even (per vertex), the
    iteration's counts, and `diagonals` = how often the two-split quad was cut [from v_j strictly, from m_j, from v_j on a tie]"""
    V, F = _mesh(V, F)
    nv, nf = len(V), len(F)
    P = V.astype(np.float64)
    faces = F.tolist()
    runs = edge_runs(F)
    thr2 = thr * thr
    # edges
    split = [len2(P[a], P[b]) > thr2 for (a, b), _ in runs]
    mid_of_entry, new_index, r = {}, [], 0
    for ((a, b), entries), s in zip(runs, split):
        new_index.append(nv + r if s else -1)
        if s:
            for e in entries:
                mid_of_entry[e] = nv + r
            r += 1
    nsplit = r
    # vertex classes
    n_border, many, at_split, border_nbrs = [0] * nv, [False] * nv, [False] * nv, [[] for _ in range(nv)]
    for ((a, b), entries), s in zip(runs, split):
        for x, y in ((a, b), (b, a)):
            if len(entries) == 1:
                n_border[x] += 1
                border_nbrs[x].append(y)
            if len(entries) >= 3:
                many[x] = True
            if s:
                at_split[x] = True
    corners = [[] for _ in range(nv)]
    for f, face in enumerate(faces):
        if distinct(face):
            for j in range(3):
                corners[face[j]].append((f, j))
    vclass = np.zeros(nv, np.int32)
    for v in range(nv):
        locked = many[v] or (n_border[v] != 0 and n_border[v] != 2) or len(corners[v]) == 0
        vclass[v] = V_LOCKED if locked else V_BORDER if n_border[v] == 2 else V_INTERIOR
    # positions
    out = np.zeros((nv + nsplit, 3), np.float32)
    moved = [0, 0]
    for v in range(nv):
        if vclass[v] == V_LOCKED or not at_split[v]:
            out[v] = V[v]
        elif vclass[v] == V_BORDER:
            p, q = border_nbrs[v]
            out[v] = (P[v] * 0.75 + (P[p] + P[q]) * 0.125).astype(np.float32)
            moved[1] += 1
        else:
            S = np.zeros(3)
            for f, j in corners[v]:
                S = S + P[faces[f][(j + 1) % 3]]
                S = S + P[faces[f][(j + 2) % 3]]
            k = len(corners[v])
            b = beta(k)
            out[v] = (P[v] * (1.0 - k * b) + (S * 0.5) * b).astype(np.float32)
            moved[0] += 1
    odd = np.zeros((len(runs), 3), np.float32)
    for i, (((a, b), entries), s) in enumerate(zip(runs, split)):
        if not s:
            continue
        if len(entries) == 2:
            c, d = (faces[e // 3][(e % 3 + 2) % 3] for e in entries)
            odd[i] = ((P[a] + P[b]) * 0.375 + (P[c] + P[d]) * 0.125).astype(np.float32)
        else:
            odd[i] = ((P[a] + P[b]) * 0.5).astype(np.float32)
        out[new_index[i]] = odd[i]
    # faces
    Q = out.astype(np.float64)
    res, patterns, diagonals = [], [0, 0, 0, 0], [0, 0, 0]
    for f, v in enumerate(faces):
        m = [mid_of_entry.get(3 * f + j, -1) for j in range(3)]
        ns = sum(1 for x in m if x >= 0)
        patterns[ns] += 1
        if ns == 0:
            res.append(v)
        elif ns == 3:
            res += [[v[0], m[0], m[2]], [m[0], v[1], m[1]], [m[2], m[1], v[2]], [m[0], m[1], m[2]]]
        elif ns == 1:
            j = [x >= 0 for x in m].index(True)
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            res += [[v[j], m[j], v[j2]], [m[j], v[j1], v[j2]]]
        else:
            j = ([x >= 0 for x in m].index(False) + 1) % 3
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            res.append([m[j], v[j1], m[j1]])
            from_v, from_m = len2(Q[v[j]], Q[m[j1]]), len2(Q[m[j]], Q[v[j2]])
            if from_v <= from_m:
                res += [[v[j], m[j], m[j1]], [v[j], m[j1], v[j2]]]
                diagonals[2 if from_v == from_m else 0] += 1
            else:
                res += [[v[j], m[j], v[j2]], [m[j], m[j1], v[j2]]]
                diagonals[1] += 1
    mult = [len(e) for _, e in runs]
    return dict(V=out, F=np.array(res, np.int32).reshape(-1, 3), keys=np.array([(a << 32) | b for (a, b), _ in runs], np.uint64),
                multiplicity=np.array(mult, np.int32), split=np.array(split, np.int32), odd=odd, vertex_class=vclass, even=out[:nv].copy(),
                n_split=nsplit, split_border=sum(1 for s, k in zip(split, mult) if s and k == 1), split_many=sum(1 for s, k in zip(split, mult) if s and k >= 3),
                patterns=patterns, diagonals=diagonals, moved_interior=moved[0], moved_border=moved[1], locked=int((vclass == V_LOCKED).sum()),
                max_valence=max([len(c) for c in corners] + [0]))


def threshold_of(V, threshold=0.0, threshold_fraction=0.0):
    return threshold_fraction * box_diagonal(V) if threshold_fraction > 0.0 else float(threshold)


def subdivide(V, F, iterations=3, threshold=0.0, threshold_fraction=0.0):
    """the whole call -> (vertices float32, faces int32, stats dict with STAT_KEYS)"""
    V, F = _mesh(V, F)
    thr = threshold_of(V, threshold, threshold_fraction)
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(n_vertices_in=len(V), n_faces_in=len(F), threshold=thr)
    if len(V) > 0 and len(F) > 0:
        for _ in range(iterations):
            w = loop_step(V, F, thr)
            st["locked_vertices"] = w["locked"]
            st["max_valence"] = max(st["max_valence"], w["max_valence"])
            if w["n_split"] == 0:
                break
            V, F = w["V"], w["F"]
            st["iterations"] += 1
            st["split_edges"] += w["n_split"]
            st["split_border_edges"] += w["split_border"]
            st["split_many_face_edges"] += w["split_many"]
            for c, k in enumerate(("faces_0_splits", "faces_1_split", "faces_2_splits", "faces_3_splits")):
                st[k] += w["patterns"][c]
            st["moved_interior"] += w["moved_interior"]
            st["moved_border"] += w["moved_border"]
    st.update(n_vertices=len(V), n_faces=len(F))
    return V.copy(), F.copy(), st


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def tetrahedron():
    return _mesh([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def octahedron():
    return _mesh([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]],
                 [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def icosahedron():
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    return _mesh(v, f)


def lattice(nx=7, ny=6):
    """a regular triangular lattice with integer coordinates: vertex (i, j) at (2 i + j, 2 j, i - j), cell (i, j) cut from (i, j) to
    (i + 1, j + 1) -- the six neighbours of an interior vertex lie in three opposite pairs, and every interior edge is the diagonal of a
    parallelogram"""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    v = np.stack([2 * i + j, 2 * j, i - j], -1).reshape(-1, 3)
    a = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)).ravel()
    return _mesh(v, np.concatenate([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)]))


def lattice_interior(nx=7, ny=6):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    return ((i > 0) & (i < nx - 1) & (j > 0) & (j < ny - 1)).ravel()


def square_patch(n=4):
    """an n x n plane of unit cells at z = 0.5, every cell cut the same way: its four corners have two border edges each"""
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    v = np.stack([i, j, np.full_like(i, 0) + 0.5], -1).reshape(-1, 3)
    a = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)).ravel()
    return _mesh(v, np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)]))


def bow_tie():
    return _mesh([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0, 2, 0.125], [1, 2, 0]], [[0, 1, 2], [2, 4, 3]])


def three_face_edge():
    return _mesh([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.25], [0.5, 0, 1]], [[0, 1, 2], [1, 0, 3], [0, 1, 4]])


PATTERN_THR = 1.5
# lone triangles (x, y of the three corners, in eighths exactly) for PATTERN_THR: the edges longer than 1.5 split
_PATTERN_TRIANGLES = (
    ("none", [(0, 0), (1, 0), (0.5, 0.875)]),
    ("one_edge0", [(0, 0), (2, 0), (1, 0.5)]),
    ("one_edge1", [(1, 0.5), (0, 0), (2, 0)]),
    ("one_edge2", [(2, 0), (1, 0.5), (0, 0)]),
    ("two_tie_keep2", [(-0.5, 0), (0, 3), (0.5, 0)]),             # the mirror image of itself: both diagonals equal
    ("two_tie_keep0", [(0.5, 0), (-0.5, 0), (0, 3)]),
    ("two_tie_keep1", [(0, 3), (0.5, 0), (-0.5, 0)]),
    ("two_from_v", [(0, 0), (-1, 3), (1, 0)]),                    # the apex leans towards v_j: v_j - m_j+1 is the shorter diagonal
    ("two_from_m", [(0, 0), (2, 3), (1, 0)]),                     # ... away from it: m_j - v_j+2 is
    ("two_from_m_rotated", [(1, 0), (0, 0), (2, 3)]),
    ("three", [(0, 0), (2, 0), (1, 2)]),
)


def pattern_mesh():
    """the lone triangles above side by side (4 apart in x, z = 0.25 k), then the pair (two triangles on one long edge, so that the two-face
    odd rule and a one-split face next to a three-split face occur), then a face with a repeated index"""
    v, f = [], []
    for k, (_, tri) in enumerate(_PATTERN_TRIANGLES):
        f.append([len(v), len(v) + 1, len(v) + 2])
        v += [[4.0 * k + x, y, 0.25 * k] for x, y in tri]
    n = len(v)
    v += [[60, 0, 0], [62, 0, 0], [61, 2, 0.5], [61, -0.5, 0]]
    f += [[n, n + 1, n + 2], [n + 1, n, n + 3], [n, n, n + 1]]
    return _mesh(v, f)


PATTERN_COUNTS = [2, 4, 6, 2]              # faces of pattern_mesh() with 0, 1, 2, 3 split edges at PATTERN_THR
PATTERN_DIAGONALS = [1, 2, 3]              # [from v_j strictly, from m_j, ties]
