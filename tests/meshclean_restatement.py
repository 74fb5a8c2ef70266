"""numpy restatement of the mesh smoothing and clean-up (reconstruction_amd/csrc/k_meshclean.hip).

Test infrastructure only: the package never imports it.  The definitions:
  edge table   a face (v0, v1, v2) with three distinct indices has edges j = (v_j, v_j+1), keyed (min << 32) | max with value 3 f + j, stably
               sorted; the incidence of an edge = its entries.  Faces with a repeated index take no part in incidences, smoothing,
               components or duplicates.  A border vertex = an endpoint of an edge of incidence 1.
  corner list  of a vertex: the values 3 f + j of the corners it is, ascending.
  smoothing    simultaneous steps on float32 positions, every sum in fp64 in the order of the corner list: an interior vertex v, corner j
               of face f, adds neighbour v_j+1 with the weight of corner j+2, then v_j+2 with the weight of corner j+1 (weight 1, or the
               cotangent clamped at 0: u = Pa - Pc, w = Pb - Pc, n2 = |u x w|^2, max(0, u.w / sqrt(n2)), 0 when n2 == 0);
               P' = float32((P + S) / (1 + W)).  A border vertex starts from S = P, W = 1 and adds the other endpoint of each incident
               edge of incidence 1 with weight 1 (boundary = 1), or stays (boundary = 0).
  clean-up     on the smoothed mesh, in script2's order: 1 components (faces connected across an edge; label = lowest face) whose float32
               box has an fp64 diameter < threshold; 2 of the faces with the same three vertices the lowest stays; 3 faces with a repeated
               index or n2 == 0 at corner 0; 4 every face on an edge that more than two of the survivors of 1-3 share; then the unused
               vertices go and both arrays are renumbered in order.
Sums run as a sequential loop over "the k-th corner of every vertex", vectorised across the vertices: numpy's reductions (np.sum,
np.add.reduceat) promise no order, this does."""
from __future__ import annotations

import numpy as np

STAT_KEYS = ("n_vertices_in", "n_faces_in", "n_vertices", "n_faces", "border_vertices", "components", "components_removed", "removed_isolated",
             "removed_duplicate", "removed_zero_area", "removed_nonmanifold", "vertices_dropped")


def _faces(faces):
    return np.asarray(faces, np.int64).reshape(-1, 3)


def distinct(faces):
    f = _faces(faces)
    return (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def edge_table(faces, alive=None):
    """(keys, values) of the sorted edge table over the faces with distinct indices (and alive, when given)"""
    f = _faces(faces)
    ok = distinct(f) if alive is None else distinct(f) & alive
    idx = np.nonzero(ok)[0]
    a, b = f[idx], f[idx][:, [1, 2, 0]]
    key = ((np.minimum(a, b) << 32) | np.maximum(a, b)).ravel()
    val = (3 * idx[:, None] + np.arange(3)).ravel()
    o = np.argsort(key, kind="stable")
    return key[o], val[o]


def incidences(faces, nv):
    """einc [3 nf] = the incidence of the edge of corner 3 f + j (0 for a face with a repeated index), border [nv] bool"""
    f = _faces(faces)
    key, val = edge_table(f)
    einc = np.zeros(3 * len(f), np.int64)
    border = np.zeros(nv, bool)
    if len(key):
        uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
        einc[val] = cnt[inv]
        one = uk[cnt == 1]
        border[one >> 32] = True
        border[one & 0xffffffff] = True
    return einc, border


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def corner_n2(pc, pa, pb):
    """(|u x w|^2, u . w) with u = pa - pc, w = pb - pc, fp64"""
    u, w = pa - pc, pb - pc
    c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    return _dot(c, c), _dot(u, w)


def corner_weight(pc, pa, pb):
    n2, d = corner_n2(pc, pa, pb)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = d / np.sqrt(n2)
    return np.where(n2 == 0.0, 0.0, np.where(c > 0.0, c, 0.0))


def corner_lists(faces, nv):
    """(start [nv + 1], corner [m]): vertex v is the corners corner[start[v]:start[v + 1]], ascending"""
    f = _faces(faces)
    idx = np.nonzero(distinct(f))[0]
    vert = f[idx].ravel()
    val = (3 * idx[:, None] + np.arange(3)).ravel()
    o = np.argsort(vert, kind="stable")
    start = np.zeros(nv + 1, np.int64)
    np.cumsum(np.bincount(vert, minlength=nv), out=start[1:])
    return start, val[o]


def smooth(verts, faces, steps, cotangent=True, boundary=True):
    """positions float32 [nv, 3] after `steps` steps"""
    P = np.array(verts, np.float32).reshape(-1, 3)
    f = _faces(faces)
    nv = len(P)
    if steps <= 0 or nv == 0 or len(f) == 0:
        return P
    einc, border = incidences(f, nv)
    start, corner = corner_lists(f, nv)
    count = np.diff(start)
    for _ in range(steps):
        P64 = P.astype(np.float64)
        S = np.where(border[:, None], P64, 0.0)
        W = np.where(border, 1.0, 0.0)
        for k in range(int(count.max()) if len(count) else 0):
            vs = np.nonzero(count > k)[0]
            c = corner[start[vs] + k]
            fi, j = c // 3, c % 3
            n1, n2 = f[fi, (j + 1) % 3], f[fi, (j + 2) % 3]
            isb = border[vs]
            # interior: neighbour v_j+1 with the weight of corner j+2, then v_j+2 with the weight of corner j+1
            q = ~isb
            v, a, b = vs[q], n1[q], n2[q]
            w1 = corner_weight(P64[b], P64[v], P64[a]) if cotangent else np.ones(len(v))
            S[v] += w1[:, None] * P64[a]
            W[v] += w1
            w2 = corner_weight(P64[a], P64[b], P64[v]) if cotangent else np.ones(len(v))
            S[v] += w2[:, None] * P64[b]
            W[v] += w2
            # border: the other endpoint of edge j = (v, v_j+1), then of edge j+2 = (v_j+2, v), where the edge has one face
            for nb, e in ((n1, 3 * fi + j), (n2, 3 * fi + (j + 2) % 3)):
                q = isb & (einc[e] == 1)
                S[vs[q]] += P64[nb[q]]
                W[vs[q]] += 1.0
        new = ((P64 + S) / (1.0 + W)[:, None]).astype(np.float32)
        P = new if boundary else np.where(border[:, None], P, new)
    return P


def components(faces):
    """(labels int32 [nf]: the lowest face index of the component, -1 for a face with a repeated index; the number of components)"""
    f = _faces(faces)
    nf = len(f)
    lab = np.arange(nf, dtype=np.int64)
    key, val = edge_table(f)
    same = key[1:] == key[:-1]
    a, b = val[1:][same] // 3, val[:-1][same] // 3
    while True:
        m = np.minimum(lab[a], lab[b])
        new = lab.copy()
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    ok = distinct(f)
    lab[~ok] = -1
    return lab.astype(np.int32), int((lab == np.arange(nf)).sum())


def box_diameter(lo, hi):
    """fp64 diameter of float32 boxes: sqrt((dx dx + dy dy) + dz dz)"""
    d = np.asarray(hi, np.float32).astype(np.float64) - np.asarray(lo, np.float32).astype(np.float64)
    d = d.reshape(-1, 3)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def component_diameters(P, faces, lab):
    """fp64 diameter of every root's box, indexed by face (nan where the face is no root)"""
    f = _faces(faces)
    nf = len(f)
    lo = np.full((nf, 3), np.inf, np.float32)
    hi = np.full((nf, 3), -np.inf, np.float32)
    ok = lab >= 0
    for c in range(3):
        np.minimum.at(lo, lab[ok], P[f[ok, c]])
        np.maximum.at(hi, lab[ok], P[f[ok, c]])
    out = np.full(nf, np.nan)
    roots = np.nonzero(lab == np.arange(nf))[0]
    out[roots] = box_diameter(lo[roots], hi[roots])
    return out


def clean(verts, faces, smooth_steps=5, cotangent=True, boundary=True, min_piece=0.10, relative=True, duplicates=True, zero_area=True,
          nonmanifold=True):
    """(vertices float32, faces int32, stats dict) -- what Context.mesh_clean returns"""
    V = np.array(verts, np.float32).reshape(-1, 3)
    f = _faces(faces)
    nv, nf = len(V), len(f)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["n_vertices_in"], st["n_faces_in"] = nv, nf
    P = smooth(V, f, smooth_steps, cotangent, boundary)
    D = float(box_diameter(P.min(0), P.max(0))[0]) if nv else 0.0
    thr = float(min_piece) * D if relative else float(min_piece)
    st["diameter"], st["threshold"] = D, thr
    if nv == 0 or nf == 0:
        st["vertices_dropped"] = nv
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), st
    st["border_vertices"] = int(incidences(f, nv)[1].sum())
    lab, ncomp = components(f)
    st["components"] = ncomp
    diam = component_diameters(P, f, lab)
    dead = diam < thr                                   # (nan compares False)
    st["components_removed"] = int(dead.sum())
    ok = distinct(f)
    r1 = ok & dead[np.where(ok, lab, 0)]
    alive = ~r1
    r2 = np.zeros(nf, bool)
    if duplicates:
        idx = np.nonzero(ok)[0]
        _, first, inv = np.unique(np.sort(f[idx], 1), axis=0, return_index=True, return_inverse=True)
        r2[idx] = first[inv.ravel()] != np.arange(len(idx))
        r2 &= alive
    alive &= ~r2
    r3 = np.zeros(nf, bool)
    if zero_area:
        P64 = P.astype(np.float64)
        n2, _ = corner_n2(P64[f[:, 0]], P64[f[:, 1]], P64[f[:, 2]])
        r3 = alive & (~ok | (n2 == 0.0))
    alive &= ~r3
    r4 = np.zeros(nf, bool)
    if nonmanifold:
        key, val = edge_table(f, alive)
        if len(key):
            uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
            r4[val[cnt[inv] > 2] // 3] = True
    alive &= ~r4
    st["removed_isolated"], st["removed_duplicate"], st["removed_zero_area"], st["removed_nonmanifold"] = (int(r.sum()) for r in (r1, r2, r3, r4))
    kf = f[alive]
    used = np.zeros(nv, bool)
    used[kf.ravel()] = True
    new = np.cumsum(used) - 1
    ov, of = P[used], new[kf].astype(np.int32).reshape(-1, 3)
    st["n_vertices"], st["n_faces"], st["vertices_dropped"] = len(ov), len(of), nv - len(ov)
    return ov, of, st


# ---- inputs the tests share ----------------------------------------------------------------------------------------------------------
def grid_mesh(nx, ny, h=1.0, z=0.0):
    """a flat regular triangulated grid of nx x ny vertices, every square cut along the same diagonal"""
    x, y = np.meshgrid(np.arange(nx) * h, np.arange(ny) * h)
    v = np.stack([x.ravel(), y.ravel(), np.full(nx * ny, z)], 1).astype(np.float32)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + nx + 1], 1), np.stack([i, i + nx + 1, i + nx], 1)])
    return v, f.astype(np.int32)


def fan_mesh(n, apex=(0.0, 0.0, 1.0), r=1.0):
    """a closed regular fan: vertex 0 = the apex over the centre of a regular n-gon of radius r in z = 0"""
    t = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([[apex], np.stack([r * np.cos(t), r * np.sin(t), np.zeros(n)], 1)]).astype(np.float32)
    f = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], 1)
    return v, f.astype(np.int32)


def cleanup_fixture(v, f):
    """The constructed clean-up fixture on a closed mesh (v, f) of some thousand faces: + a copy scaled to 5 % and one scaled to 20 %, both
    moved clear of it by its largest extent (along x and along y), three duplicated faces (as it is, rotated, reversed), a face with a
    repeated index, a collinear face of its own (inside the mesh, 0.4 extents long: too long to go as an isolated piece at 10 %), and a fin
    on edge (v0, v1) of face 10.  Returns (vertices, faces, expect), expect = the faces each rule must remove with the default parameters:
    the whole 5 % copy; the three duplicates; the repeated index and the collinear face; face 10, its neighbour across the edge and the fin."""
    v = np.asarray(v, np.float32)
    f = np.asarray(f, np.int32)
    nv, nf = len(v), len(f)
    c = v.astype(np.float64).mean(0)
    ext = float((v.max(0).astype(np.float64) - v.min(0)).max())
    small = ((v - c) * 0.05 + c + np.array([ext, 0.0, 0.0])).astype(np.float32)
    mid = ((v - c) * 0.20 + c + np.array([0.0, ext, 0.0])).astype(np.float32)
    p0 = (c - np.array([0.2 * ext, 0.0, 0.0])).astype(np.float32)
    col = np.stack([p0, p0 + np.float32([0.2 * ext, 0.0, 0.0]), p0 + np.float32([0.4 * ext, 0.0, 0.0])]).astype(np.float32)   # y, z equal: n2 = 0 exactly
    a, b = int(f[10][0]), int(f[10][1])
    fin = (c + (v[a].astype(np.float64) - c) * 1.5).astype(np.float32)[None]                                            # a point outside the surface
    V = np.concatenate([v, small, mid, col, fin]).astype(np.float32)
    i_col, i_fin = 3 * nv, 3 * nv + 3
    F = np.concatenate([f, f + nv, f + 2 * nv,
                        [f[3], f[4][[1, 2, 0]], f[5][[0, 2, 1]]],
                        [[f[6][0], f[6][0], f[6][1]]],
                        [[i_col, i_col + 1, i_col + 2]],
                        [[a, b, i_fin]]]).astype(np.int32)
    return V, F, dict(removed_isolated=nf, removed_duplicate=3, removed_zero_area=2, removed_nonmanifold=3)
