"""numpy restatement of the hole closing (reconstruction_amd/csrc/k_meshclose.hip).

Test infrastructure only: the package never imports it.  The definitions (the project's own; not MeshLab's):
  border entry  the edge table is f8's: a face with three distinct indices has entries e = 3 f + j keyed (min << 32) | max of (v_j, v_j+1);
                e is a border entry when no other entry has its key.  tail(e) = v_j, head(e) = v_j+1.  out(v) / in(v) count the border
                entries with tail / head v; v is simple when both are 1.
  components    border entries e, e' are linked when head(e) = tail(e') = v and v is simple; label = the lowest entry.  A component is
                a loop when the head of every entry is simple (one cycle of length L = its entries), else open (never closed).
  eligible      a loop with L <= max_hole_size that is not a lone triangle (L = 3, its three entries from one face).
  ring          e0 = the label: r_0 = head(e0), r_1 = tail(e0), r_t+1 = tail(the border entry whose head is r_t): the border against the
                faces' direction, so that a fill (r_i, r_k, r_j), i < k < j, is oriented like its neighbours.
  forbidden     F(i, j), i + 2 <= j, (i, j) != (0, L - 1): the key of (r_i, r_j) is in the input's edge table.
  triangulation W(i, i+1) = 0; for spans 2 .. L - 1: W(i, j) = +inf, K = -1 if F(i, j), else the least over k = i+1 .. j-1 of
                (W(i, k) + W(k, j)) + A(i, k, j), strict < from +inf in ascending k; A = 0.5 sqrt(n2), u = P_k - P_i, w = P_j - P_i in fp64,
                c = u x w with each product rounded, n2 = (c0^2 + c1^2) + c2^2; n2 == 0: the triangle is inadmissible (+inf).
                W(0, L - 1) = +inf: the hole stays whole.
  output        vertices and input faces untouched; new faces appended, holes in ascending label, within a hole the pre-order of
                emit(0, L - 1): emit(i, j) = nothing when j - i < 2, else k = K(i, j): (r_i, r_k, r_j), emit(i, k), emit(k, j).
Every fp64 operation is a Python float operation (IEEE double, no fused multiply-add) in the order written."""
from __future__ import annotations

import itertools
import math

import numpy as np

STAT_KEYS = ("n_vertices_in", "n_faces_in", "n_faces", "border_entries", "components", "loops", "open_components", "loops_closed", "loops_too_long",
             "lone_triangles", "loops_untriangulated", "faces_added", "longest_closed", "longest_loop")
INF = float("inf")


def _faces(faces):
    return np.asarray(faces, np.int64).reshape(-1, 3)


def edge_keys(faces):
    """(key [3 nf] of entry 3 f + j, -1 for a face with a repeated index; the set of keys)"""
    f = _faces(faces)
    ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    a, b = f, f[:, [1, 2, 0]]
    key = np.where(ok[:, None], (np.minimum(a, b) << 32) | np.maximum(a, b), -1).ravel()
    return key, set(key[key >= 0].tolist())


def border_loops(faces, nv):
    """rules 2-3: dict with label [3 nf] (-1: no border entry), size [3 nf] (L for a loop's entries, 0 for an open component's, -1
    otherwise), components (label -> sorted entries), loops (label -> ring of vertex indices), open (labels), in_entry / out_entry"""
    f = _faces(faces)
    n = 3 * len(f)
    key, _ = edge_keys(f)
    count = {}
    for k in key.tolist():
        if k >= 0:
            count[k] = count.get(k, 0) + 1
    border = [e for e in range(n) if key[e] >= 0 and count[int(key[e])] == 1]
    tail = f.ravel()
    head = f[:, [1, 2, 0]].ravel()
    n_in, n_out, in_entry, out_entry = np.zeros(nv, np.int64), np.zeros(nv, np.int64), {}, {}
    for e in border:
        n_out[tail[e]] += 1
        n_in[head[e]] += 1
        out_entry[int(tail[e])] = e
        in_entry[int(head[e])] = e
    simple = (n_in == 1) & (n_out == 1)
    parent = {e: e for e in border}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for e in border:
        if simple[head[e]]:
            a, b = find(e), find(out_entry[int(head[e])])
            if a != b:
                parent[max(a, b)] = min(a, b)
    comps = {}
    for e in border:
        comps.setdefault(find(e), []).append(e)
    label, size = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    loops, opened = {}, []
    for lab in sorted(comps):
        es = comps[lab]
        assert lab == min(es)
        is_loop = all(simple[head[e]] for e in es)
        label[es] = lab
        size[es] = len(es) if is_loop else 0
        if not is_loop:
            opened.append(lab)
            continue
        L = len(es)
        ring = [int(head[lab]), int(tail[lab])]
        while len(ring) < L:
            ring.append(int(tail[in_entry[ring[-1]]]))
        assert L >= 3 and len(set(ring)) == L and int(tail[in_entry[ring[-1]]]) == ring[0]
        loops[lab] = ring
    return dict(label=label, size=size, components=comps, loops=loops, open=opened, n_border=len(border))


def tri_n2(pi, pk, pj):
    """|(P_k - P_i) x (P_j - P_i)|^2 of three points given as tuples of Python floats"""
    u0, u1, u2 = pk[0] - pi[0], pk[1] - pi[1], pk[2] - pi[2]
    w0, w1, w2 = pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]
    c0, c1, c2 = u1 * w2 - u2 * w1, u2 * w0 - u0 * w2, u0 * w1 - u1 * w0
    return (c0 * c0 + c1 * c1) + c2 * c2


def tri_area(pi, pk, pj):
    """A(i, k, j), +inf for a triangle without area"""
    n2 = tri_n2(pi, pk, pj)
    return INF if n2 == 0.0 else 0.5 * math.sqrt(n2)


def _points(ring_xyz):
    p = np.asarray(ring_xyz, np.float32).reshape(-1, 3)
    return [tuple(float(x) for x in row) for row in p]


def triangulate(ring_xyz, forbidden=None):
    """rule 7 and rule 8's order on a ring of L float32 points; forbidden: None or an L x L array read at [i, j], i + 2 <= j, (i, j) != (0, L-1).
    Returns (W(0, L-1), triangles int32 [L-2, 3] of ring positions -- [0, 3] when there is no triangulation)"""
    P = _points(ring_xyz)
    L = len(P)
    assert L >= 3
    W = [[0.0] * L for _ in range(L)]
    K = [[-1] * L for _ in range(L)]
    for s in range(2, L):
        for i in range(L - s):
            j = i + s
            best, bk = INF, -1
            if not (forbidden is not None and (i, j) != (0, L - 1) and forbidden[i][j]):
                for k in range(i + 1, j):
                    c = (W[i][k] + W[k][j]) + tri_area(P[i], P[k], P[j])
                    if c < best:
                        best, bk = c, k
            W[i][j], K[i][j] = best, bk
    if W[0][L - 1] == INF:
        return INF, np.zeros((0, 3), np.int32)
    tris = []

    def emit(i, j):
        if j - i < 2:
            return
        k = K[i][j]
        tris.append((i, k, j))
        emit(i, k)
        emit(k, j)
    emit(0, L - 1)
    assert len(tris) == L - 2
    return W[0][L - 1], np.array(tris, np.int32)


def all_triangulations(i, j):
    """every triangulation of the polygon i .. j as a list of triangles (i, k, j)"""
    if j - i < 2:
        return [[]]
    out = []
    for k in range(i + 1, j):
        for a in all_triangulations(i, k):
            for b in all_triangulations(k, j):
                out.append([(i, k, j)] + a + b)
    return out


def brute_force(ring_xyz, forbidden=None):
    """the least total area over all admissible triangulations, each triangulation's areas summed in fp64 (any order: compare with a
    tolerance of a few ulps), and how many are admissible"""
    P = _points(ring_xyz)
    L = len(P)
    best, admissible = INF, 0
    for tris in all_triangulations(0, L - 1):
        total, ok = 0.0, True
        for (i, k, j) in tris:
            a = tri_area(P[i], P[k], P[j])
            diag = [(x, y) for x, y in ((i, k), (k, j), (i, j)) if y - x >= 2 and (x, y) != (0, L - 1)]
            if a == INF or (forbidden is not None and any(forbidden[x][y] for x, y in diag)):
                ok = False
                break
            total += a
        if ok:
            admissible += 1
            best = min(best, total)
    return best, admissible


def close_holes(verts, faces, max_hole_size=30):
    """rules 1-9: (vertices (the input's), faces int32 [nf + added, 3], stats dict, info dict: closed = {label: ring}, skipped labels by cause)"""
    assert 3 <= max_hole_size <= 64
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(v), len(f)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["n_vertices_in"], st["n_faces_in"], st["n_faces"] = nv, nf, nf
    info = dict(closed={}, too_long=[], lone=[], untriangulated=[])
    if nv == 0 or nf == 0:
        return v, f, st, info
    b = border_loops(f, nv)
    _, keys = edge_keys(f)
    st["border_entries"], st["components"], st["loops"], st["open_components"] = b["n_border"], len(b["components"]), len(b["loops"]), len(b["open"])
    new = []
    for lab in sorted(b["loops"]):
        ring = b["loops"][lab]
        L = len(ring)
        st["longest_loop"] = max(st["longest_loop"], L)
        if L > max_hole_size:
            st["loops_too_long"] += 1
            info["too_long"].append(lab)
            continue
        if L == 3 and len({e // 3 for e in b["components"][lab]}) == 1:
            st["lone_triangles"] += 1
            info["lone"].append(lab)
            continue
        F = [[False] * L for _ in range(L)]
        for i in range(L):
            for j in range(i + 2, L):
                if (i, j) != (0, L - 1):
                    F[i][j] = ((min(ring[i], ring[j]) << 32) | max(ring[i], ring[j])) in keys
        w, tris = triangulate(v[ring], F)
        if w == INF:
            st["loops_untriangulated"] += 1
            info["untriangulated"].append(lab)
            continue
        st["loops_closed"] += 1
        st["longest_closed"] = max(st["longest_closed"], L)
        info["closed"][lab] = ring
        new.append(np.asarray(ring, np.int32)[tris])
    if new:
        f = np.ascontiguousarray(np.concatenate([f] + new), np.int32)
    st["faces_added"] = len(f) - nf
    st["n_faces"] = len(f)
    return v, f, st, info


# ---- post-conditions by plain counting ----------------------------------------------------------------------------------------------------------
def directed_counts(faces):
    """{(a, b): faces that hold the directed edge a -> b}, faces with a repeated index left out"""
    d = {}
    for t in _faces(faces).tolist():
        if len(set(t)) == 3:
            for j in range(3):
                e = (t[j], t[(j + 1) % 3])
                d[e] = d.get(e, 0) + 1
    return d


def undirected_counts(faces):
    u = {}
    for (a, b), c in directed_counts(faces).items():
        k = (min(a, b), max(a, b))
        u[k] = u.get(k, 0) + c
    return u


def check_closed(v, f, fo, info):
    """what closing the loops of info["closed"] must have done to (v, f), counted without the restatement's tables"""
    nf = len(f)
    assert np.array_equal(fo[:nf], f)
    before, after = undirected_counts(f), undirected_counts(fo)
    d = directed_counts(fo)
    total = 0
    for lab, ring in info["closed"].items():
        L = len(ring)
        total += L
        for t in range(L):                                                        # the ring runs against the faces: the border entry is r_t+1 -> r_t
            a, b = ring[(t + 1) % L], ring[t]
            assert before[(min(a, b), max(a, b))] == 1 and d[(a, b)] == 1 and d[(b, a)] == 1
    assert sum(1 for c in before.values() if c == 1) - sum(1 for c in after.values() if c == 1) == total
    assert all(c <= 2 for k, c in after.items() if before.get(k, 0) <= 2)
    P = np.asarray(v, np.float64)
    old = {frozenset(t) for t in f.tolist()}
    new = fo[nf:].tolist()
    assert len({frozenset(t) for t in new}) == len(new) == sum(len(r) - 2 for r in info["closed"].values())
    for t in new:
        assert frozenset(t) not in old and tri_n2(tuple(P[t[0]]), tuple(P[t[1]]), tuple(P[t[2]])) > 0.0
    return total


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def plane(nx, ny, flip=False):
    """a regular nx x ny plane of vertices at z = 0, cell (i, j) = faces c and (nx-1)(ny-1) + c with c = j (nx - 1) + i:
    (a, a+1, a+nx+1) and (a, a+nx+1, a+nx), a = j nx + i"""
    X, Y = np.meshgrid(np.arange(nx), np.arange(ny))
    v = np.stack([X.ravel(), Y.ravel(), np.zeros(nx * ny)], 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1))
    a = (j * nx + i).ravel()
    f = np.concatenate([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)])
    if flip:
        f = f[:, ::-1]
    return v, np.ascontiguousarray(f, np.int32)


def remove_faces(f, drop):
    keep = np.ones(len(f), bool)
    keep[list(drop)] = False
    return np.ascontiguousarray(f[keep])


def faces_of_vertex(f, v):
    return np.nonzero((f == v).any(1))[0].tolist()


def cut_plane():
    """the 9 x 9 plane with three cuts: one triangle (L = 3), the two of a cell (L = 4), the fan of vertex 58 (L = 6, the vertex left
    unreferenced); jittered in z so that no fill is flat.  (vertices, faces)"""
    v, f = plane(9, 9)
    rng = np.random.default_rng(12)
    v[:, 2] = rng.uniform(-0.3, 0.3, len(v)).astype(np.float32)
    cells = 8 * 8
    drop = [1 * 8 + 1] + [1 * 8 + 5, cells + 1 * 8 + 5] + faces_of_vertex(f, 6 * 9 + 4)
    return v, remove_faces(f, drop)


def annulus(L, jitter=0.05, seed=3):
    """an inner ring of L vertices (radius 1) and an outer ring of 2 L (radius 2), 3 L faces between them, counter-clockwise seen from +z;
    non-planar: every vertex is moved by up to `jitter`.  The inner border is a loop of L, the outer one of 2 L."""
    rng = np.random.default_rng(seed + L)
    a = 2.0 * np.pi * np.arange(L) / L
    b = 2.0 * np.pi * (np.arange(2 * L) - 0.5) / (2 * L)
    v = np.concatenate([np.stack([np.cos(a), np.sin(a), 0 * a], 1), np.stack([2 * np.cos(b), 2 * np.sin(b), 0 * b], 1)])
    v = (v + rng.uniform(-jitter, jitter, v.shape)).astype(np.float32)
    f = []
    for i in range(L):
        i1, o0, o1, o2 = (i + 1) % L, L + 2 * i, L + (2 * i + 1) % (2 * L), L + (2 * i + 2) % (2 * L)
        f += [(i, o0, o1), (i, o1, i1), (i1, o1, o2)]
    return v, np.array(f, np.int32)


def ring_points(L, seed=0, jitter=0.2):
    """L float32 points around a circle, moved off their plane and along it"""
    rng = np.random.default_rng(1000 * seed + L)
    a = 2.0 * np.pi * np.arange(L) / L
    p = np.stack([np.cos(a), np.sin(a), 0 * a], 1) * (1.0 + 0.05 * L)
    return (p + rng.uniform(-jitter, jitter, p.shape)).astype(np.float32)


def collinear_hole():
    """the 5 x 5 plane without the triangle (6, 7, 12), vertex 7 moved onto the line through the other two: a loop of 3 whose only
    triangulation has no area"""
    v, f = plane(5, 5)
    assert f[5].tolist() == [6, 7, 12]
    v[7] = (1.5, 1.5, 0.0)
    return v, remove_faces(f, [5])


TETRA_V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
TETRA_F = np.int32([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])   # outward


def many_holes(nx=41, ny=31, seed=5):
    """the nx x ny plane with one-triangle and two-triangle holes in every second cell of every second row (266 of them, no two sharing a vertex), z jittered"""
    v, f = plane(nx, ny)
    rng = np.random.default_rng(seed)
    v[:, 2] = rng.uniform(-0.3, 0.3, len(v)).astype(np.float32)
    cells = (nx - 1) * (ny - 1)
    drop, holes = [], 0
    for j in range(1, ny - 2, 2):
        for i in range(1, nx - 2, 2):
            c = j * (nx - 1) + i
            kind = int(rng.integers(0, 3))
            drop += [c] if kind == 0 else [cells + c] if kind == 1 else [c, cells + c]
            holes += 1
    return v, remove_faces(f, drop), holes
