"""The rules of the mesh decimation (csrc/k_meshdecimate.hip) restated in numpy: decimation.mlx's "Quadric Edge Collapse
Decimation", not a bit-parity port of MeshLab / VCG.  The kernels are held to this file exactly (tests/test_gpu_meshdecimate.py: the same
faces in the same order, the same float32 positions, the same fp64 quadrics and costs), and this file to known answers and invariants
(tests/test_meshdecimate_cpu.py).  Every fp64 expression is written with the parentheses the kernels use; every sum has a stated order.

Quadric entries, in this order: xx xy xz xd yy yz yd zz zd dd of the plane (n, d)'s outer product.
Reject codes (the low four bits of `reject`; the first rule that fails): 0 candidate, 1 an edge of more than two faces, 2 a locked
endpoint, 3 the link condition's count of common neighbours, 4 both endpoints on the border but the edge not, 5 two surviving faces with
the same vertices, 6 a face's normal turned over (preserve_normal), 7 an error or cost that is not finite.  Bits 4-5 hold the placement
branch where a position was computed (codes 0, 6, 7): 0 the solve's optimum, 1 Pa, 2 Pb, 3 the midpoint."""
import math

import numpy as np

K_QUALITY = 3.4641016151377544  # 2 sqrt(3)
NO_RANK = 0xFFFFFFFF
R_OK, R_NONMANIFOLD, R_LOCKED, R_LINK, R_BORDER, R_DUPLICATE, R_NORMAL, R_NOTFINITE = range(8)
B_OPTIMAL, B_PA, B_PB, B_MID = range(4)
STAT_KEYS = ("n_vertices_in", "n_faces_in", "n_vertices", "n_faces", "repeated_index_faces", "rounds", "collapses", "border_collapses",
             "rejected_nonmanifold", "rejected_locked", "rejected_link", "rejected_border", "rejected_duplicate", "rejected_normal",
             "rejected_not_finite", "locked_vertices", "max_valence", "max_cost", "target_reached", "target")


def params(target_faces=100000, target_fraction=0.0, quality_thr=0.3, preserve_boundary=0, boundary_weight=1.0, preserve_normal=0,
           preserve_topology=1, optimal_placement=1, min_error=1e-15, max_rounds=1000):
    return dict(target_faces=int(target_faces), target_fraction=float(target_fraction), quality_thr=float(quality_thr),
                preserve_boundary=int(preserve_boundary), boundary_weight=float(boundary_weight), preserve_normal=int(preserve_normal),
                preserve_topology=int(preserve_topology), optimal_placement=int(optimal_placement), min_error=float(min_error),
                max_rounds=int(max_rounds))


def _arrays(V, F):
    return np.ascontiguousarray(V, np.float32).reshape(-1, 3), np.ascontiguousarray(F, np.int32).reshape(-1, 3)


def distinct(F):
    return (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])


class Tables:
    """The sorted edge table and the corner lists of the faces without a repeated index."""

    def __init__(self, F, nv):
        F = F.astype(np.int64)
        self.nv, self.F = nv, F
        ok = distinct(F)
        self.ok = ok
        fi = np.nonzero(ok)[0]
        # entries 3 f + j of edge j = (v_j, v_j+1)
        ent = (3 * fi[:, None] + np.arange(3)[None, :]).ravel()
        a = F[fi][:, [0, 1, 2]].ravel()
        b = F[fi][:, [1, 2, 0]].ravel()
        key = np.minimum(a, b) * (1 << 32) + np.maximum(a, b)
        self.ukey, inv, self.mult = np.unique(key, return_inverse=True, return_counts=True)
        self.ua, self.ub = self.ukey >> 32, self.ukey & 0xFFFFFFFF
        self.entry_border = np.zeros(3 * len(F), bool)     # per entry: its edge is in exactly one face
        self.entry_border[ent] = self.mult[inv] == 1
        # corner lists: per vertex the corners 3 f + j that hold it, ascending
        cv = F[fi].ravel()
        order = np.argsort(cv, kind="stable")              # (ent is ascending)
        self.corner = ent[order]
        self.row = np.zeros(nv + 1, np.int64)
        np.cumsum(np.bincount(cv, minlength=nv), out=self.row[1:])
        self.valence = np.diff(self.row)
        self.vborder = np.zeros(nv, bool)
        m1 = self.mult == 1
        self.vborder[self.ua[m1]] = True
        self.vborder[self.ub[m1]] = True

    def star_rows(self, verts):
        """(index into verts, corner) for every corner in the lists of verts, in list order."""
        cnt = self.valence[verts]
        idx = np.repeat(np.arange(len(verts)), cnt)
        start = np.repeat(self.row[verts], cnt)
        within = np.arange(len(idx)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        return idx, self.corner[start + within]


def _plane_quadric(n, d):
    """[m,3], [m] -> [m,10]"""
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    return np.stack([nx * nx, nx * ny, nx * nz, nx * d, ny * ny, ny * nz, ny * d, nz * nz, nz * d, d * d], axis=1)


def _cross(u, w):
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)


def _dot(u, w):
    return (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2]


def _border_quadric(n, Pa, Pb, bw):
    """The plane through the directed edge (a, b) perpendicular to the face with normal n; zeros for an edge without length."""
    e = Pb - Pa
    L = np.sqrt(_dot(e, e))
    c = _cross(n, e)
    with np.errstate(all="ignore"):
        m = (bw * c) / L[:, None]
        q = _plane_quadric(m, -_dot(m, Pa))
    q[L == 0.0] = 0.0
    return q, L != 0.0


def quadrics(V, F, boundary_weight=1.0, tables=None):
    """Q_v [nv,10] fp64: the sum from 0 over v's corner list, ascending; per corner the face's quadric, then the border quadric of edge j,
    then that of edge (j+2)%3, where they are border edges."""
    V, F = _arrays(V, F)
    nv = len(V)
    T = tables or Tables(F, nv)
    P = V.astype(np.float64)
    Q = np.zeros((nv, 10))
    if len(T.corner) == 0:
        return Q
    with np.errstate(all="ignore"):
        c = T.corner
        f, j = c // 3, c % 3
        vert = T.F[f, j]
        P0, P1, P2 = P[T.F[f, 0]], P[T.F[f, 1]], P[T.F[f, 2]]
        n = _cross(P1 - P0, P2 - P0)
        Kf = _plane_quadric(n, -_dot(n, P0))
        j1, j2 = (j + 1) % 3, (j + 2) % 3
        qa, ha = _border_quadric(n, P[T.F[f, j]], P[T.F[f, j1]], boundary_weight)     # edge j = (v_j, v_j+1)
        ha &= T.entry_border[3 * f + j]
        qb, hb = _border_quadric(n, P[T.F[f, j2]], P[T.F[f, j]], boundary_weight)     # edge j+2 = (v_j+2, v_j)
        hb &= T.entry_border[3 * f + j2]
        # the contributions in order: slot 0 the face, 1 edge j, 2 edge j+2
        m = len(c)
        vals = np.stack([Kf, qa, qb], axis=1).reshape(3 * m, 10)
        has = np.stack([np.ones(m, bool), ha, hb], axis=1).ravel()
        vs = np.repeat(vert, 3)[has]
        vals = vals[has]
        # k-th contribution of every vertex at once (vs is grouped by vertex: the corner lists are)
        cnt = np.bincount(vs, minlength=nv)
        start = np.cumsum(cnt) - cnt
        k = np.arange(len(vs)) - start[vs]
        for kk in range(int(k.max()) + 1):
            s = k == kk
            Q[vs[s]] = Q[vs[s]] + vals[s]
    return Q


def _qerr(Q, x):
    """v^T Q v for v = (x, 1), in the kernels' order."""
    X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
    r0 = ((Q[:, 0] * X + Q[:, 1] * Y) + Q[:, 2] * Z) + Q[:, 3]
    r1 = ((Q[:, 1] * X + Q[:, 4] * Y) + Q[:, 5] * Z) + Q[:, 6]
    r2 = ((Q[:, 2] * X + Q[:, 5] * Y) + Q[:, 7] * Z) + Q[:, 8]
    r3 = ((Q[:, 3] * X + Q[:, 6] * Y) + Q[:, 8] * Z) + Q[:, 9]
    return ((X * r0 + Y * r1) + Z * r2) + r3


def _f32(x):
    with np.errstate(all="ignore"):
        return x.astype(np.float32)


def placement(Q, Pa, Pb, optimal):
    """-> (float32 position [m,3], branch [m]).  Every candidate position is rounded to float32 first and judged as that."""
    m = len(Q)
    with np.errstate(all="ignore"):
        mid = (Pa + Pb) * 0.5
        midf = _f32(mid)
        pos = np.zeros((m, 3), np.float32)
        ea = _qerr(Q, Pa)
        eb = _qerr(Q, Pb)
        em = _qerr(Q, midf.astype(np.float64))
        branch = np.full(m, B_PA)
        best = ea.copy()
        pos[:] = _f32(Pa)
        s = eb < best
        branch[s], best[s], pos[s] = B_PB, eb[s], _f32(Pb)[s]
        s = em < best
        branch[s], pos[s] = B_MID, midf[s]
        if optimal:
            q0, q1, q2, q3, q4, q5, q6, q7, q8 = (Q[:, i] for i in range(9))
            c00 = q4 * q7 - q5 * q5
            c01 = q2 * q5 - q1 * q7
            c02 = q1 * q5 - q4 * q2
            c11 = q0 * q7 - q2 * q2
            c12 = q1 * q2 - q0 * q5
            c22 = q0 * q4 - q1 * q1
            det = (q0 * c00 + q1 * c01) + q2 * c02
            x = np.stack([-(((c00 * q3 + c01 * q6) + c02 * q8) / det), -(((c01 * q3 + c11 * q6) + c12 * q8) / det),
                          -(((c02 * q3 + c12 * q6) + c22 * q8) / det)], axis=1)
            xf = _f32(x)
            xd = xf.astype(np.float64)
            d = xd - mid
            e = Pb - Pa
            ok = np.isfinite(det) & (det != 0.0) & np.isfinite(xf).all(axis=1) & (_dot(d, d) <= 4.0 * _dot(e, e))
            branch[ok] = B_OPTIMAL
            pos[ok] = xf[ok]
    return pos, branch


def collapse_costs(V, F, Q, p, tables=None):
    """Per unique edge in key order: key (uint64), multiplicity, cost (+inf: no candidate), reject, position (float32 [ne,3]); and the tables."""
    V, F = _arrays(V, F)
    nv = len(V)
    T = tables or Tables(F, nv)
    P = V.astype(np.float64)
    Q = np.asarray(Q, np.float64).reshape(nv, 10)
    ne = len(T.ukey)
    ua, ub, mult = T.ua, T.ub, T.mult
    locked = np.zeros(nv, bool)
    nm = mult > 2
    locked[ua[nm]] = True
    locked[ub[nm]] = True
    if p["preserve_boundary"]:
        locked |= T.vborder
    T.locked = locked
    reject = np.zeros(ne, np.int64)
    cost = np.full(ne, np.inf)
    pos = np.zeros((ne, 3), np.float32)
    if ne == 0:
        return T.ukey.astype(np.uint64), mult.astype(np.int32), cost, reject.astype(np.int32), pos, T

    def first(mask, code):
        reject[(reject == 0) & mask] = code

    first(nm, R_NONMANIFOLD)
    first(locked[ua] | locked[ub], R_LOCKED)
    # the stars: corners of a and of b
    ia, ca = T.star_rows(ua)
    ib, cb = T.star_rows(ub)
    Fa, Fb = T.F[ca // 3], T.F[cb // 3]
    sa = ~(Fa == ub[ia][:, None]).any(axis=1)              # surviving faces of a's star: those without b
    sb = ~(Fb == ua[ib][:, None]).any(axis=1)
    if p["preserve_topology"]:
        # common neighbours: c next to a (a vertex of a face at a) that is next to b as well
        adj = np.unique(np.concatenate([T.ukey, ub * (1 << 32) + ua]))
        na_v = np.repeat(ua[ia], 2)
        j = ca % 3
        na_c = np.stack([Fa[np.arange(len(ca)), (j + 1) % 3], Fa[np.arange(len(ca)), (j + 2) % 3]], axis=1).ravel()
        pairs = np.unique(np.stack([np.repeat(ia, 2), na_c], axis=1), axis=0)     # (edge, distinct neighbour of a)
        want = ub[pairs[:, 0]] * (1 << 32) + pairs[:, 1]
        at = np.searchsorted(adj, want)
        hit = (at < len(adj)) & (adj[np.minimum(at, len(adj) - 1)] == want)
        common = np.bincount(pairs[hit, 0], minlength=ne)
        first(common != mult, R_LINK)
        first(T.vborder[ua] & T.vborder[ub] & (mult != 1), R_BORDER)
    # two surviving faces with the same vertices: a face at a without b whose triple with b for a is some face's triple
    tri = np.sort(T.F[T.ok], axis=1)
    pk = tri[:, 0] * nv + tri[:, 1]
    up = np.unique(pk)
    fk = np.sort(np.searchsorted(up, pk) * nv + tri[:, 2])
    A = Fa[sa].copy()
    ea_idx = ia[sa]
    A[A == ua[ea_idx][:, None]] = -1
    A = np.where(A < 0, ub[ea_idx][:, None], A)
    A = np.sort(A, axis=1)
    qp = A[:, 0] * nv + A[:, 1]
    i1 = np.searchsorted(up, qp)
    ok1 = (i1 < len(up)) & (up[np.minimum(i1, len(up) - 1)] == qp)
    qk = i1 * nv + A[:, 2]
    i2 = np.searchsorted(fk, qk)
    ok2 = ok1 & (i2 < len(fk)) & (fk[np.minimum(i2, len(fk) - 1)] == qk)
    dup = np.bincount(ea_idx[ok2], minlength=ne) > 0
    first(dup, R_DUPLICATE)
    # placement and error for the edges still standing
    live = reject == 0
    with np.errstate(all="ignore"):
        Qe = Q[ua] + Q[ub]
        Pa, Pb = P[ua], P[ub]
        pos, branch = placement(Qe, Pa, Pb, p["optimal_placement"])
        x = pos.astype(np.float64)
        err = _qerr(Qe, x)
        # the surviving faces of both stars with x put in: normals and quality
        idx = np.concatenate([ia[sa], ib[sb]])
        faces = np.concatenate([Fa[sa], Fb[sb]])
        moved = np.concatenate([ua[ia[sa]], ub[ib[sb]]])
        O = [P[faces[:, k]] for k in range(3)]
        N = [np.where((faces[:, k] == moved)[:, None], x[idx], O[k]) for k in range(3)]
        n_old = _cross(O[1] - O[0], O[2] - O[0])
        n_new = _cross(N[1] - N[0], N[2] - N[0])
        flip = ~(_dot(n_new, n_old) > 0.0)
        flipped = np.bincount(idx[flip], minlength=ne) > 0
        nn = _dot(n_new, n_new)
        e0, e1, e2 = N[1] - N[0], N[2] - N[1], N[0] - N[2]
        s = (_dot(e0, e0) + _dot(e1, e1)) + _dot(e2, e2)
        q = np.where((nn > 0.0) & (s > 0.0), (K_QUALITY * np.sqrt(nn)) / s, 0.0)
        minq = np.ones(ne)
        np.minimum.at(minq, idx, q)
        if p["preserve_normal"]:
            first(flipped, R_NORMAL)
        first(~np.isfinite(err), R_NOTFINITE)
        err = np.where(err > p["min_error"], err, p["min_error"])
        if p["quality_thr"] > 0.0:
            cl = np.where(minq < 1e-8, 1e-8, minq)
            cl = np.where(cl > p["quality_thr"], p["quality_thr"], cl)
            c = err / cl
        else:
            c = err
        first(~np.isfinite(c), R_NOTFINITE)
    cand = reject == 0
    cost[cand] = c[cand]
    pos[~live] = 0.0
    reject = np.where(live, reject | (branch << 4), reject)
    return T.ukey.astype(np.uint64), mult.astype(np.int32), cost, reject.astype(np.int32), pos, T


def collapse_round(V, F, Q, need, p):
    """One round, a pure function of (float32 V, int32 F, fp64 Q, need) -> dict(V, F, Q, selected (keys in priority order), kept, ...)."""
    V, F = _arrays(V, F)
    nv = len(V)
    Q = np.asarray(Q, np.float64).reshape(nv, 10)
    key, mult, cost, reject, pos, T = collapse_costs(V, F, Q, p)
    ne = len(key)
    out = dict(V=V.copy(), F=F[distinct(F)].copy(), Q=Q.copy(), selected=np.zeros(0, np.uint64), kept=0, removed=0, border_kept=0, max_cost=0.0,
               rejects=np.bincount(reject & 15, minlength=8)[:8], locked=int(T.locked.sum()) if ne else 0,
               max_valence=int(T.valence.max()) if nv else 0, edges=ne)
    if ne == 0 or need <= 0:
        return out
    order = np.argsort(cost.view(np.uint64), kind="stable")
    rank = np.empty(ne, np.int64)
    rank[order] = np.arange(ne)
    part = np.isfinite(cost) & (rank < (need + 1) // 2)
    ua, ub = T.ua, T.ub
    m1 = np.full(nv, NO_RANK, np.int64)
    np.minimum.at(m1, ua[part], rank[part])
    np.minimum.at(m1, ub[part], rank[part])
    m2 = m1.copy()
    np.minimum.at(m2, ua, m1[ub])
    np.minimum.at(m2, ub, m1[ua])
    sel = part & (rank == m2[ua]) & (rank == m2[ub])
    so = order[sel[order]]                                  # the selected edges in rank order
    scan = np.cumsum(mult[so]) - mult[so]
    ko = so[scan < need]
    a, b = ua[ko], ub[ko]
    out["selected"], out["kept"] = key[so], len(ko)
    out["V"][a] = pos[ko]
    out["Q"][a] = Q[a] + Q[b]
    vmap = np.arange(nv)
    vmap[b] = a
    F2 = vmap[F].astype(np.int32)
    F2 = F2[distinct(F2)]
    out["removed"] = len(out["F"]) - len(F2)
    out["F"] = F2
    out["border_kept"] = int((mult[ko] == 1).sum())
    out["max_cost"] = float(cost[ko].max()) if len(ko) else 0.0
    return out


def resolve_target(p, nf):
    return int(math.floor(p["target_fraction"] * nf)) if p["target_fraction"] > 0.0 else p["target_faces"]


def decimate(V, F, p):
    """The whole call -> (V float32, F int32, stats dict)."""
    V, F = _arrays(V, F)
    nv_in, nf_in = len(V), len(F)
    target = resolve_target(p, nf_in)
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(n_vertices_in=nv_in, n_faces_in=nf_in, target=target, max_cost=0.0)
    keep = distinct(F)
    st["repeated_index_faces"] = int((~keep).sum())
    F = F[keep]
    if len(F) > target:
        Q = quadrics(V, F, p["boundary_weight"])
        while len(F) > target and st["rounds"] < p["max_rounds"]:
            r = collapse_round(V, F, Q, len(F) - target, p)
            st["rounds"] += 1
            for c, k in enumerate(STAT_KEYS[8:15]):
                st[k] = int(r["rejects"][c + 1])
            st["locked_vertices"] = r["locked"]
            st["max_valence"] = max(st["max_valence"], r["max_valence"])
            if r["kept"] == 0:
                break
            st["collapses"] += r["kept"]
            st["border_collapses"] += r["border_kept"]
            st["max_cost"] = max(st["max_cost"], r["max_cost"])
            V, F, Q = r["V"], r["F"], r["Q"]
    used = np.zeros(nv_in, bool)
    used[F.ravel()] = True
    vpos = np.cumsum(used) - used
    Vo = V[used]
    Fo = vpos[F].astype(np.int32).reshape(-1, 3)
    st.update(n_vertices=len(Vo), n_faces=len(Fo), target_reached=int(len(Fo) <= target))
    return np.ascontiguousarray(Vo, np.float32), Fo, st


# ---- the meshes of the tests (shared by both files, so that what the CPU tests assert holds for what the GPU tests use) -----------------------
def grid_mesh(n, height=None, jitter=0.0, seed=0):
    """An n x n vertex grid over [0, n-1]^2, two triangles a cell; height(x, y) or flat; the interior jittered in the plane."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    if jitter > 0.0:
        inner = np.zeros((n, n), bool)
        inner[1:-1, 1:-1] = True
        x = x + inner * rng.uniform(-jitter, jitter, (n, n))
        y = y + inner * rng.uniform(-jitter, jitter, (n, n))
    z = np.zeros_like(x) if height is None else height(x, y)
    V = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    v00 = (i * n + j).ravel()
    v10, v01, v11 = v00 + n, v00 + 1, v00 + n + 1
    F = np.stack([np.stack([v00, v10, v11], axis=1), np.stack([v00, v11, v01], axis=1)], axis=1).reshape(-1, 3).astype(np.int32)
    return V, F


def bumpy(x, y):
    return 0.8 * np.sin(0.9 * x) * np.cos(0.7 * y) + 0.05 * x


def icosphere(levels):
    t = (1.0 + math.sqrt(5.0)) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, np.float64) / math.sqrt(1 + t * t) for v in V]
    for _ in range(levels):
        cache, F2 = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                cache[k] = len(V) - 1
            return cache[k]

        for a, b, c in F:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            F2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = F2
    return np.array(V, np.float32), np.array(F, np.int32)


TETRA = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32))
OCTA = (np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32),
        np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32))
# three faces on the edge (0, 1)
FAN3 = (np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -1, 0.2], [0.5, 0, 1], [1.5, 1, 0.3]], np.float32),
        np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [1, 5, 2]], np.int32))
# two triangles that share vertex 2 only
BOWTIE = (np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0, 2, 0.1], [1, 2, 0]], np.float32), np.array([[0, 1, 2], [2, 4, 3]], np.int32))


def corner_mesh(origin=(1.0, 2.0, 3.0)):
    """Three mutually orthogonal squares of 2 x 2 cells that meet in a corner (vertex 0, at origin), two triangles a cell; the vertices next
    to the corner along the axes are 1 = +x, 2 = +y, 3 = +z, none of them on the border."""
    index, V, F = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(V)
            V.append(p)
        return index[p]

    for p in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        vid(p)
    for axis in range(3):                                  # the square in the plane where coordinate `axis` is 0
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for i in range(2):
            for j in range(2):
                def pt(a, b):
                    q = [0, 0, 0]
                    q[u], q[w] = a, b
                    return vid(tuple(q))
                F += [(pt(i, j), pt(i + 1, j), pt(i + 1, j + 1)), (pt(i, j), pt(i + 1, j + 1), pt(i, j + 1))]
    return (np.array(V, np.float64) + np.array(origin)).astype(np.float32), np.array(F, np.int32)


def edge_counts(F):
    F = np.asarray(F, np.int64).reshape(-1, 3)
    a, b = F[:, [0, 1, 2]].ravel(), F[:, [1, 2, 0]].ravel()
    return np.unique(np.minimum(a, b) * (1 << 32) + np.maximum(a, b), return_counts=True)


def border_loops(F):
    """The number of closed loops the border edges form (every border vertex of the test meshes has two of them)."""
    k, c = edge_counts(F)
    k = k[c == 1]
    a, b = (k >> 32).tolist(), (k & 0xFFFFFFFF).tolist()
    nxt = {}
    for u, w in zip(a, b):
        nxt.setdefault(u, []).append(w)
        nxt.setdefault(w, []).append(u)
    seen, loops = set(), 0
    for s in nxt:
        if s in seen:
            continue
        loops += 1
        stack = [s]
        while stack:
            u = stack.pop()
            if u in seen:
                continue
            seen.add(u)
            stack += nxt[u]
    return loops


# ---- the whole-call cases of the GPU tests: (name, mesh, params); tests/test_meshdecimate_cpu.py asserts that each ends at target or target - 1 ----
def whole_cases():
    hv, hf = grid_mesh(21, bumpy)
    iv, if_ = icosphere(3)
    return [("height_field_20pc", (hv, hf), params(target_fraction=0.2)), ("icosphere_320", (iv, if_), params(target_faces=320)),
            ("height_field_160", (hv, hf), params(target_faces=160)),
            ("height_field_normals", (hv, hf), params(target_faces=200, preserve_normal=1, quality_thr=0.0)),
            ("plane_boundary", grid_mesh(9, None, 0.3), params(target_faces=60, preserve_boundary=1, boundary_weight=4.0)),
            ("height_field_endpoints", (hv, hf), params(target_faces=400, optimal_placement=0, preserve_topology=0))]
