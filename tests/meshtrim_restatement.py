"""numpy restatement of the density trim of the Poisson surface (reconstruction_amd/csrc/k_meshtrim.hip).

Test infrastructure only: the package never imports it.  The definitions, in DESIGN's numbering:
  1 samples, grid  f7's valid samples (without normals: a finite point is enough) and f7's o and side; the density grid has Nk = 2^kernel_depth
                   nodes per axis at o + (i + 1/2) hk, hk = side / Nk.
  2 count splat    C(node) += llrint(w 2^32), trilinear over 8 nodes (corner order dz, dy, dx, dx fastest; w = (wx wy) wz), outside dropped;
                   Python integers.
  3 value          rho(v) = the same eight weights at (v - o) / hk - 1/2 times C 2^-32, summed in that corner order (C = 0 outside);
                   value = max(0, kernel_depth + 1/2 log2(rho / samples_per_node)), 0 when rho = 0.
  4 smoothing      value'_i = (value_i + S_i) / (1 + m_i), S_i = the values of i's incidences summed from 0.0 in the order of its corner
                   list (per corner f[(j+1)%3], then f[(j+2)%3]); m_i = 0: the value stays.
  5 split          keep(v) = value_v >= trim.  A cut edge (lo < hi, keep differs) gets the vertex float32(P_lo + t (P_hi - P_lo)),
                   t = (trim - value_lo) / (value_hi - value_lo); cut vertices are numbered nv + rank in ascending (lo << 32) | hi.  A face
                   with one corner a alone on its side (cyclic a, b, c) becomes (a, ab, ca) on a's side and the quad (ab, b, c, ca) on the
                   other, cut along its shorter diagonal: |q1 - q3|^2 < |q0 - q2|^2 gives (q0, q1, q3), (q1, q2, q3), else (q0, q1, q2),
                   (q0, q2, q3).  Faces with a repeated index are dropped.
  6 islands        components per side over the split mesh's sorted edge table (label = the lowest triangle); q = llrint(area 2^32 / D^2),
                   area = 1/2 sqrt(|u x w|^2) with u = P1 - P0, w = P2 - P0; a component that holds a triangle of a split face and has
                   float(Q_c) < island_ratio float(Q_total) changes side.
  7 output         the kept triangles in (source face, triangle) order; the original vertices in use, then the cut vertices in use.
Sums whose order is part of a rule run as sequential loops (vectorised across vertices, as meshclean_restatement does)."""
from __future__ import annotations

import math

import numpy as np

import meshclean_restatement as mr
import poisson_restatement as pr

FIX = 4294967296.0   # 2^32
STAT_KEYS = ("n_vertices_in", "n_faces_in", "n_vertices", "n_faces", "n_valid", "n_invalid", "cut_edges", "faces_split", "repeated_index_faces",
             "zero_area_triangles", "components_kept", "components_dropped", "moved_to_dropped", "moved_to_kept", "q_total")


# ---- 1-3: density ------------------------------------------------------------------------------------------------------------------------
def valid_points(xyz, normals=None):
    """fp64 positions of the valid samples and the valid mask: f7's rule, or with normals None a finite point"""
    if normals is not None:
        p, _, ok = pr.valid_samples(xyz, normals)
        return p, ok
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    ok = np.isfinite(xyz).all(1)
    return xyz[ok].astype(np.float64), ok


def resolve_kernel_depth(depth, kernel_depth=0):
    return depth - 2 if kernel_depth == 0 else kernel_depth


def density_grid(p, depth, scale, kernel_depth):
    """(o [3], hk) of the density grid, or None: no valid sample or all points equal"""
    g = pr.make_grid(p, depth, scale)
    if g is None:
        return None
    o, h = g
    side = h * float(1 << depth)                      # (a power of two: exact both ways)
    return o, side / float(1 << kernel_depth)


def count_splat(p, o, hk, kernel_depth):
    """C as a list of Nk^3 Python integers (fixed point, scale 2^32)"""
    Nk = 1 << kernel_depth
    C = [0] * (Nk ** 3)
    idx, w, ok = pr._trilinear(p, o, hk, Nk)
    lin = idx[..., 0] + Nk * (idx[..., 1] + Nk * idx[..., 2])
    for s in range(len(p)):
        for c in range(8):
            if ok[s, c]:
                C[int(lin[s, c])] += int(np.rint(w[s, c] * FIX))
    return C


def density(samples_xyz, samples_normals, verts, depth, scale=1.1, kernel_depth=0, samples_per_node=2.0):
    """(rho [nv], value [nv], (valid, invalid)) at the float32 vertices"""
    kd = resolve_kernel_depth(depth, kernel_depth)
    V = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    p, ok = valid_points(samples_xyz, samples_normals)
    counts = (int(ok.sum()), int(len(ok) - ok.sum()))
    rho = np.zeros(len(V))
    g = density_grid(p, depth, scale, kd)
    if g is not None and len(V):
        o, hk = g
        Nk = 1 << kd
        C = count_splat(p, o, hk, kd)
        Cf = np.array([float(c) for c in C]) / FIX
        idx, w, inside = pr._trilinear(V, o, hk, Nk)
        lin = np.where(inside, idx[..., 0] + Nk * (idx[..., 1] + Nk * idx[..., 2]), 0)
        for c in range(8):
            rho = rho + np.where(inside[:, c], w[:, c] * Cf[lin[:, c]], 0.0)
    value = np.zeros(len(V))
    for i in range(len(V)):
        if rho[i] > 0.0:
            value[i] = max(0.0, float(kd) + 0.5 * math.log2(rho[i] / samples_per_node))
    return rho, value, counts


# ---- 4: smoothing ------------------------------------------------------------------------------------------------------------------------
def neighbours(faces, nv):
    """(start [nv + 1], nbr [2 m]): vertex i's incidences nbr[start[i]:start[i + 1]] in the rule's order"""
    f = mr._faces(faces)
    cstart, corner = mr.corner_lists(f, nv)
    fi, j = corner // 3, corner % 3
    nbr = np.stack([f[fi, (j + 1) % 3], f[fi, (j + 2) % 3]], 1).ravel() if len(corner) else np.zeros(0, np.int64)
    return 2 * cstart, nbr


def value_smooth(values, faces, steps):
    x = np.array(values, np.float64).reshape(-1)
    nv = len(x)
    if steps <= 0 or nv == 0:
        return x
    start, nbr = neighbours(faces, nv)
    m = np.diff(start)
    for _ in range(steps):
        S = np.zeros(nv)
        for k in range(int(m.max()) if nv else 0):
            vs = np.nonzero(m > k)[0]
            S[vs] = S[vs] + x[nbr[start[vs] + k]]
        x = np.where(m > 0, (x + S) / (1.0 + m), x)
    return x


# ---- 5-7: split, islands, output -------------------------------------------------------------------------------------------------------------
def _d2(a, b):
    d = a - b
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def _n2(p0, p1, p2):
    return float(mr.corner_n2(p0[None], p1[None], p2[None])[0][0])


def split(verts, faces, values, trim, island_ratio=0.0):
    """The whole of rules 5-7.  Returns a dict: vertices float32 [., 3], faces int32 [., 3] (the output), src / side / label per output face,
    stats, and the split mesh itself: split_vertices, split_faces, split_src, split_side (before rule 6), split_label, split_final,
    cut_keys (ascending), q (per split triangle), Q (per label)."""
    P = np.array(verts, np.float32).reshape(-1, 3)
    f = mr._faces(faces)
    x = np.asarray(values, np.float64).reshape(-1)
    nv = len(P)
    keep = x >= trim
    ok = mr.distinct(f)
    # cut edges, ascending key
    key, _ = mr.edge_table(f)
    uk = np.unique(key)
    lo, hi = uk >> 32, uk & 0xffffffff
    cut = keep[lo] != keep[hi] if len(uk) else np.zeros(0, bool)
    cut_keys = uk[cut]
    rank = {int(k): nv + r for r, k in enumerate(cut_keys)}
    SV = np.zeros((nv + len(cut_keys), 3), np.float32)
    SV[:nv] = P
    P64 = P.astype(np.float64)
    for k, r in rank.items():
        a, b = k >> 32, k & 0xffffffff
        t = (trim - x[a]) / (x[b] - x[a])
        SV[r] = (P64[a] + t * (P64[b] - P64[a])).astype(np.float32)
    S64 = SV.astype(np.float64)

    def cutv(a, b):
        return rank[(min(a, b) << 32) | max(a, b)]

    T, src, side, zero_area, faces_split = [], [], [], 0, 0
    for fi in range(len(f)):
        if not ok[fi]:
            continue
        v = [int(q) for q in f[fi]]
        k = [bool(keep[q]) for q in v]
        if k[0] == k[1] == k[2]:
            T.append(v), src.append(fi), side.append(int(k[0]))
            continue
        faces_split += 1
        j = [j for j in range(3) if k[j] != k[(j + 1) % 3] and k[j] != k[(j + 2) % 3]][0]
        a, b, c = v[j], v[(j + 1) % 3], v[(j + 2) % 3]
        ab, ca = cutv(a, b), cutv(c, a)
        q0, q1, q2, q3 = ab, b, c, ca
        tris = [(a, ab, ca)]
        tris += [(q0, q1, q3), (q1, q2, q3)] if _d2(S64[q1], S64[q3]) < _d2(S64[q0], S64[q2]) else [(q0, q1, q2), (q0, q2, q3)]
        for n, t3 in enumerate(tris):
            T.append(list(t3)), src.append(fi), side.append(int(k[j]) if n == 0 else int(k[(j + 1) % 3]))
            zero_area += _n2(S64[t3[0]], S64[t3[1]], S64[t3[2]]) == 0.0
    T = np.array(T, np.int64).reshape(-1, 3)
    src, side = np.array(src, np.int64), np.array(side, np.int64)
    nT = len(T)
    # components per side: along each run of the split mesh's edge table a triangle joins the nearest earlier one of its side
    parent = list(range(nT))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    skey, sval = mr.edge_table(T) if nT else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    for i in range(1, len(skey)):
        q = i - 1
        while q >= 0 and skey[q] == skey[i]:
            ta, tb = int(sval[i] // 3), int(sval[q] // 3)
            if side[ta] == side[tb]:
                ra, rb = find(ta), find(tb)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
                break
            q -= 1
    label = np.array([find(t) for t in range(nT)], np.int64)
    # areas in fixed point
    D2 = 0.0
    if nv:
        ext = P64.max(0) - P64.min(0)
        D2 = float((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2])
    was_split = np.zeros(len(f), bool)
    if nT:
        was_split[src] = np.bincount(src, minlength=len(f))[src] == 3
    q = [0] * nT
    Q, touches = {}, {}
    if D2 > 0.0:
        for t in range(nT):
            area = 0.5 * math.sqrt(_n2(S64[T[t, 0]], S64[T[t, 1]], S64[T[t, 2]]))
            q[t] = int(np.rint((area * FIX) / D2))
    for t in range(nT):
        Q[int(label[t])] = Q.get(int(label[t]), 0) + q[t]
        touches[int(label[t])] = touches.get(int(label[t]), False) or bool(was_split[src[t]])
    Q_total = sum(Q.values())
    moves = {c: False for c in Q}
    if island_ratio > 0.0 and D2 > 0.0 and Q_total > 0:
        for c in Q:
            moves[c] = touches[c] and float(Q[c]) < island_ratio * float(Q_total)
    final = np.array([side[t] ^ int(moves[int(label[t])]) for t in range(nT)], np.int64)
    roots = sorted(Q)
    # output
    kept = np.nonzero(final == 1)[0]
    used = np.zeros(len(SV), bool)
    used[T[kept].ravel()] = True
    renum = np.cumsum(used) - 1
    stats = dict(n_vertices_in=nv, n_faces_in=len(f), n_vertices=int(used.sum()), n_faces=len(kept), n_valid=0, n_invalid=0, cut_edges=len(cut_keys),
                 faces_split=faces_split, repeated_index_faces=int((~ok).sum()), zero_area_triangles=int(zero_area),
                 components_kept=sum(1 for c in roots if side[c] == 1), components_dropped=sum(1 for c in roots if side[c] == 0),
                 moved_to_dropped=sum(1 for c in roots if moves[c] and side[c] == 1), moved_to_kept=sum(1 for c in roots if moves[c] and side[c] == 0),
                 q_total=Q_total)
    return dict(vertices=SV[used], faces=renum[T[kept]].astype(np.int32).reshape(-1, 3), src=src[kept].astype(np.int32), side=side[kept].astype(np.int32),
                label=label[kept].astype(np.int32), stats=stats, split_vertices=SV, split_faces=T, split_src=src, split_side=side, split_label=label,
                split_final=final, cut_keys=cut_keys, q=q, Q=Q, D2=D2)


def trim_mesh(verts, faces, samples_xyz, samples_normals, depth, scale=1.1, kernel_depth=0, samples_per_node=2.0, smooth_steps=100, trim=7.0,
              island_ratio=0.01, values=None):
    """The whole call; values: the density stage's values from elsewhere (the GPU's, for the whole-call test), else this restatement's"""
    rho, value, counts = density(samples_xyz, samples_normals, verts, depth, scale, kernel_depth, samples_per_node)
    x = value_smooth(value if values is None else values, faces, smooth_steps)
    out = split(verts, faces, x, trim, island_ratio)
    out["stats"].update(n_valid=counts[0], n_invalid=counts[1])
    out["values"] = x
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
def plane(nx, ny, step=1.0, flip=False):
    """a regular nx x ny plane of vertices at z = 0, two triangles per cell: (vertices float32, faces int32)"""
    X, Y = np.meshgrid(np.arange(nx) * step, np.arange(ny) * step)
    v = np.stack([X.ravel(), Y.ravel(), np.zeros(nx * ny)], 1).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1))
    a = (j * nx + i).ravel()
    f = np.concatenate([np.stack([a, a + 1, a + nx + 1], 1), np.stack([a, a + nx + 1, a + nx], 1)])
    if flip:
        f = f[:, ::-1]
    return v, np.ascontiguousarray(f, np.int32)


def tetra_sphere(levels=3, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """a closed sphere by `levels` 1:4 subdivisions of a tetrahedron, outward faces"""
    v = [np.array(p, np.float64) / math.sqrt(3.0) for p in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
    f = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    V = (np.array(v) * radius + np.array(centre)).astype(np.float32)
    F = np.array(f, np.int32)
    c = V[F].astype(np.float64)
    out = (np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]) * (c.mean(1) - np.array(centre))).sum(1)
    F[out < 0] = F[out < 0][:, ::-1]
    return V, F


def cap_samples(n=2000, seed=7):
    """about n samples of a spherical cap (pole -z, centre pr.SPHERE_C, radius 50) whose density falls toward the rim, outward normals"""
    rng = np.random.default_rng(seed)
    th = np.abs(rng.normal(size=n)) * 0.45            # polar angle from -z: dense at the pole, sparse at the rim
    th = th[th < 1.25]
    ph = rng.uniform(0.0, 2.0 * math.pi, size=len(th))
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], 1)
    return pr._with_normals(pr.SPHERE_C + pr.SPHERE_R * d, d)


def island_scene():
    """(vertices, faces, values, names): a 101 x 81 plane, kept (8) for x < 70 and dropped (6) beyond; inside the kept region a low disc of
    about 0.3 % of the area (vertices within 2.6 of (20, 20); the cut runs half an edge further out) and one of about 5 % (within 11 of
    (45, 50)); inside the dropped region a high disc of 0.3 % (within 2.6 of (85, 40)); beside the plane two small closed spheres, one wholly above trim, one wholly below.
    names maps what each piece is to a point inside it."""
    v, f = plane(101, 81)
    x, y = v[:, 0].astype(np.float64), v[:, 1].astype(np.float64)
    val = np.where(x < 70.0, 8.0, 6.0)
    val[(x - 20.0) ** 2 + (y - 20.0) ** 2 < 2.6 ** 2] = 6.0
    val[(x - 45.0) ** 2 + (y - 50.0) ** 2 < 11.0 ** 2] = 6.0
    val[(x - 85.0) ** 2 + (y - 40.0) ** 2 < 2.6 ** 2] = 8.0
    s1v, s1f = tetra_sphere(2, 2.0, (20.0, 95.0, 0.0))
    s2v, s2f = tetra_sphere(2, 2.0, (60.0, 95.0, 0.0))
    V = np.concatenate([v, s1v, s2v])
    F = np.concatenate([f, s1f + len(v), s2f + len(v) + len(s1v)]).astype(np.int32)
    val = np.concatenate([val, np.full(len(s1v), 9.0), np.full(len(s2v), 5.0)])
    names = dict(small_low_disc=(20.0, 20.0), big_low_disc=(45.0, 50.0), small_high_disc=(85.0, 40.0), high_sphere=(20.0, 95.0), low_sphere=(60.0, 95.0))
    return V, F, val, names


_island = {}


def island_result(ratio):
    """(vertices, faces, values, names, split(...)) of the island scene, computed once per ratio and shared by the tests that read it"""
    if ratio not in _island:
        V, F, val, names = island_scene()
        _island[ratio] = (V, F, val, names, split(V, F, val, 7.0, ratio))
    return _island[ratio]
