"""Probe clouds for the radius-cell grid of the cloud searches (csrc/cloud_grid.h: the filter's k-nearest ladder and radius
normals, the MLS).  Test infrastructure only.

A query walks the 27 cells around its own; that is correct only if every point the membership test accepts -- float32
(dx*dx + dy*dy) + dz*dz <= fl(h*h) for the k nearest, < fl32(r*r) with h = fl32(r) for the radius searches -- lies at most one
cell away on each axis.  This module restates in numpy how the grid assigns cells, under two rules:
  OLD    floorf(fl32(v - o) * fl32(1 / h)), cell edge h (the rule before the fix): its rounding of v - o and of the product puts
         some pairs at a float distance below r into cells two apart -- the search then loses a neighbour;
  FIXED  floor(fl64(fl64(v - o) * fl64(1 / H))), H = grid_edge(h) = h (1 + 2^-20) (the bound next to cell_of).
Both clamp to [0, n - 1] with n = min(2^20, floor(extent / edge) + 1) cells per axis, origin = the box's low corner.

The generators build small clouds of clusters around pairs that the membership test accepts but the OLD rule puts two cells
apart, each cluster sized so that the lost point changes the result (a neighbour count of exactly 3, or 6 for an order-2 MLS fit;
for the k nearest, the lost point among the k + 1 nearest of a query the level still decides), and assert that they did.
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
CAP = 1 << 20                     # most cells per axis (build_grid)
ORIGINS = (0.0, -37.25, 1e3 + 0.3, 1e5 + 0.3, -(1e3 + 0.3), -(1e5 + 0.3))
RADII = (2.5, 8.0, 2.3, 0.7, 0.1)


# ---- the membership tests -------------------------------------------------------------------------------------------
def fdist2(p, q):
    """float32 (dx*dx + dy*dy) + dz*dz of fdist2 / oracle/cloud_oracle.c's dist2f, broadcasting over [..., 3]."""
    p, q = np.asarray(p, F32), np.asarray(q, F32)
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def accept(d2, r, kind):
    """kind "radius": d2 < fl32(r*r) (normals, MLS; the grid's h = fl32(r)); "knn": d2 <= fl(h*h), h = fl32(r) (the ladder)."""
    if kind == "radius":
        return d2 < F32(float(r) * float(r))
    h = F32(r)
    return d2 <= h * h


# ---- the two cell rules -----------------------------------------------------------------------------------------------
def grid_edge(h):
    """cloud_grid.h grid_edge: the FIXED rule's cell edge for search radius h (float32), in double."""
    H = float(F32(h)) * (1.0 + 2.0 ** -20)
    return max(H, 2.0 ** -62)


def dims(rule, h, lo, hi):
    """Cells per axis of build_grid for the box [lo, hi] (float32 corners)."""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    if rule == "old":
        ext = (hi - lo).astype(F64)                       # (double)(bb_hi - bb_lo): the float difference
        n = np.floor(ext / float(F32(h))) + 1.0
    else:
        n = np.floor((hi.astype(F64) - lo.astype(F64)) / grid_edge(h)) + 1.0
    return np.minimum(CAP, np.maximum(1.0, n)).astype(np.int64)


def cells(rule, v, o, h, n):
    """cell_of of coordinates v (float32) against origin o, n cells (broadcasting)."""
    v, o = np.asarray(v, F32), np.asarray(o, F32)
    if rule == "old":
        inv = F32(1.0) / F32(h)
        t = ((v - o) * inv).astype(F64)                   # float32 subtraction and product, then floorf
    else:
        t = (v.astype(F64) - o.astype(F64)) * (1.0 / grid_edge(h))
    return np.clip(np.floor(t), 0, np.asarray(n, F64) - 1).astype(np.int64)


def found(rule, P, Q, h, lo, n):
    """Whether Q lies in the 27 cells around P (both [..., 3]) on the grid with low corner lo and n cells per axis."""
    ok = np.ones(np.broadcast_shapes(np.shape(P)[:-1], np.shape(Q)[:-1]), bool)
    for a in range(3):
        ok &= np.abs(cells(rule, np.asarray(P)[..., a], lo[a], h, n[a]) - cells(rule, np.asarray(Q)[..., a], lo[a], h, n[a])) <= 1
    return ok


# ---- 1-D sweep: accepted pairs the rule puts two or more cells apart ----------------------------------------------------
def _ulps(x, k):
    """the floats x - k ulp .. x + k ulp, [len(x), 2k + 1]"""
    b = np.asarray(x, F32).reshape(-1).view(np.int32).astype(np.int64)
    s = np.where(b < 0, -1, 1)                            # sign-magnitude: step the magnitude (not across zero)
    steps = np.arange(-k, k + 1)
    m = np.maximum((b & 0x7fffffff)[:, None] + s[:, None] * steps[None, :], 0)
    return (np.where(b[:, None] < 0, m | -0x80000000, m)).astype(np.int32).view(F32)


def straddles(rule, r, o, js, kind, n=CAP, k=24):
    """Pairs (a, b) of float32 coordinates, a near the cell boundaries o + j h and o + j grid_edge(h) for j in js and b within the
    membership test of a (1-D: the two other axes agree), that the rule puts two or more cells apart.  (Each fl(d_a^2) is at most
    the 3-D fdist2, so a 1-D pair is the worst case of an axis.)  Returns float32 [m, 2]."""
    h = float(F32(r))
    js = np.asarray(js, F64)
    centres = np.concatenate([F64(o) + js * h, F64(o) + js * grid_edge(r)]).astype(F32)
    A = _ulps(centres, k).ravel()
    A = A[np.isfinite(A)]
    out = []
    for sgn in (1.0, -1.0):
        B = _ulps((A.astype(F64) + sgn * h).astype(F32), k)   # [len(A), 2k + 1]
        with np.errstate(all="ignore"):
            d = (B - A[:, None]).astype(F32)
            ok = accept(d * d, r, kind) & np.isfinite(B)
        B = np.where(ok, B, A[:, None])
        gap = np.abs(cells(rule, B, o, r, n) - cells(rule, A[:, None], o, r, n))
        i, j = np.nonzero(ok & (gap >= 2))
        out.append(np.stack([A[i], B[i, j]], 1))
    res = np.concatenate(out).astype(F32)
    return np.unique(res, axis=0) if len(res) else res.reshape(0, 2)


def sweep_js(rng, count=400, n=CAP):
    """Cell boundaries to probe: the first cells, powers of two, the cap, and a log-uniform sample up to it."""
    fixed = [1, 2, 3, 5, 12, 13, 41, 100, 1000, 1 << 12, 1 << 16, 1 << 19, n - 3, n - 2, n - 1]
    return np.unique(np.concatenate([fixed, np.exp(rng.uniform(0.0, np.log(n - 1), count)).astype(np.int64)]))


# ---- clouds -----------------------------------------------------------------------------------------------------------
def neighbour_counts(xyz, r, kind, lo, n, h=None):
    """Per point: accepted neighbours (itself included) by brute force and those the OLD rule's 27 cells hold."""
    h = r if h is None else h
    xyz = np.asarray(xyz, F32)
    true = np.zeros(len(xyz), np.int64)
    old = np.zeros(len(xyz), np.int64)
    for s in range(0, len(xyz), 256):
        P = xyz[s:s + 256, None, :]
        acc = accept(fdist2(P, xyz[None]), r, kind)
        true[s:s + 256] = acc.sum(1)
        old[s:s + 256] = (acc & found("old", P, xyz[None], h, lo, n)).sum(1)
    return true, old


def _pairs_for(r, o, kind, rng, need, jmax, jmin=1, lim=None):
    """Straddling pairs under the OLD rule with cells j in [jmin, jmax), at most one per boundary."""
    js = np.unique(np.concatenate([np.arange(jmin, min(jmax, jmin + 400)),
                                   np.exp(rng.uniform(np.log(max(jmin, 1)), np.log(jmax), 3000)).astype(np.int64)]))
    js = js[(js >= jmin) & (js < jmax - 3)]
    pr = straddles("old", r, o, js, kind, n=CAP)
    h = float(F32(r))
    jj = np.floor((pr[:, 0].astype(F64) - F64(F32(o))) / h + 0.5).astype(np.int64)
    _, first = np.unique(jj, return_index=True)
    pr = pr[first]
    rng.shuffle(pr)
    return pr[:lim] if lim else pr


def radius_probe_cloud(r, o, seed=0, jmax=None, clusters=60, order2=True, far=None, expect_loss=True):
    """A cloud for the radius searches (normals, MLS) at radius r whose bounding box starts at o on every axis: an anchor point at
    the corner, then one row of cells (in y) per cluster.  Cluster kind 3: p, q (the accepted pair the OLD rule puts two cells apart,
    along x) and w beside p -- p has exactly 3 neighbours, 2 in the OLD grid.  Kind 6 (order2): p, q and four points beside p on a
    curved sheet -- 6 neighbours, an order-2 fit; 5 in the OLD grid.  far: an extra anchor (x) that stretches the box, e.g. past the
    2^20-cell cap (expect_loss = False: a box that clamps every probe into one cell loses nothing).  Returns (xyz float32 [n, 3],
    info dict)."""
    rng = np.random.default_rng(seed)
    h = float(F32(r))
    o32 = F32(o)
    jmax = jmax or int(min(CAP - 8, 2e6))
    pairs = _pairs_for(r, o, "radius", rng, clusters, jmax, lim=clusters)
    assert len(pairs) > 0, ("no straddling pair", r, o)
    pts = [[o32, o32, o32]]
    kinds = []
    z0 = float(o32) + 1.5 * h
    row = 0
    for i, (a, b) in enumerate(pairs):
        for kind in ((3, 6) if order2 else (3,)):
            y = float(o32) + (4 * row + 1.5) * h
            row += 1
            p, q = [a, y, z0], [b, y, z0]
            s = 1.0 if b > a else -1.0                      # the side of p away from q: -s
            if kind == 3:
                ext = [[a, y + 0.6 * h, z0 + 0.05 * h]]
            else:                                          # a curved sheet z = z0 + 0.3 (dx^2 + dy^2) / h
                offs = [(-0.5, 0.0), (-0.3, 0.5), (0.0, -0.6), (-0.2, -0.4)]
                ext = [[a + s * dx * h, y + dy * h, z0 + 0.3 * (dx * dx + dy * dy) * h] for dx, dy in offs]
            pts += [p, q] + ext
            kinds += [kind] * (2 + len(ext))
    if far is not None:
        pts.append([far, o32, o32])
    xyz = np.asarray(pts, F32)
    lo, hi = xyz.min(0), xyz.max(0)
    n = dims("old", r, lo, hi)
    true, old = neighbour_counts(xyz, r, "radius", lo, n)
    lost3 = int(((true >= 3) != (old >= 3)).sum())
    lost6 = int(((true >= 6) != (old >= 6)).sum())
    if expect_loss:
        assert lost3 > 0, ("no probe loses the 3-neighbour rule", r, o)
        assert lost6 > 0 or not order2, ("no probe loses the 6-neighbour fit", r, o)
    return xyz, dict(pairs=len(pairs), lost3=lost3, lost6=lost6, lost=int((true != old).sum()), cells=n, lo=lo)


def knn_probe_cloud(h, o, k=1, seed=0, span=(60, 24, 24), jmax=None, clusters=40, anchors=None):
    """A cloud for the k-nearest ladder with its first level's search radius pinned to h: anchor stacks (duplicates) at both
    corners of the box o .. o + span * h -- more than 1 % of the points each, so the filter's robust box is the exact one and
    the level's origin is o -- and clusters along x: p, q (the accepted pair the OLD rule puts two cells apart) and k points beside p
    at float distances strictly between |p q| and h (their square roots differ from |p q|'s), in the middle of their cells.  The
    level decides p in the OLD grid too (k + 1 points within h), with a wrong k-th neighbour.  Returns (xyz, info)."""
    rng = np.random.default_rng(seed)
    h32 = F32(h)
    hh = float(h32)
    h2 = h32 * h32
    o32 = F32(o)
    span = np.asarray(span, F64)
    lo = np.full(3, o32, F32)
    hi = (F64(o32) + span * hh).astype(F32)
    n_old = dims("old", h, lo, hi)
    jmax = int(min(jmax or n_old[0], n_old[0]))
    pairs = _pairs_for(h, o, "knn", rng, clusters, jmax, jmin=2)
    pts, made = [], 0
    ny, nz = int(n_old[1]), int(n_old[2])
    for a, b in pairs:
        if made >= clusters:
            break
        d2q = F32(b - a) * F32(b - a)
        # rows of cells in (y, z) for this cluster: a new one each, away from the box's faces
        cy, cz = 2 + (3 * made) % max(1, ny - 6), 2 + 3 * ((3 * made) // max(1, ny - 6)) % max(1, nz - 6)
        y = F32(F64(o32) + (cy + 0.5) * hh)
        z = F32(F64(o32) + (cz + 0.5) * hh)
        ext = []
        # k points at distances in (|p q|, h]: along +y, -y, +z, -z from p (each lands mid-cell one cell over)
        for ax, sg in ((1, 1.0), (1, -1.0), (2, 1.0), (2, -1.0)):
            if len(ext) == k:
                break
            base = y if ax == 1 else z
            for c in _ulps(np.array([F64(base) + sg * hh], F32), 64)[0][::-1 if sg > 0 else 1]:
                e = F32(c - base)
                e2 = e * e
                if d2q < e2 <= h2 and np.sqrt(e2) != np.sqrt(d2q) and all(e2 != x[1] for x in ext):
                    pt = [a, y, z]
                    pt[ax] = c
                    ext.append((pt, e2))
                    break
        if len(ext) < k:
            continue
        pts += [[a, y, z], [b, y, z]] + [pt for pt, _ in ext]
        made += 1
    assert made > 0, ("no k-nearest probe", h, o)
    body = np.asarray(pts, F32)
    m = anchors or max(8, int(0.04 * len(body)) + 2)
    xyz = np.concatenate([np.repeat(lo[None], m, 0), body, np.repeat(hi[None], m, 0)]).astype(F32)
    info = knn_route_losses(xyz, h, k, lo, n_old)
    assert info["wrong"] > 0, ("no k-nearest probe decided wrongly", h, o, info)
    info.update(clusters=made, cells_old=n_old, lo=lo, hi=hi)
    return xyz, info


def knn_route_losses(xyz, h, k, lo, n):
    """The first ladder level (search radius h, the OLD grid with low corner lo and n cells) on xyz, query by query against brute
    force: how many queries it decides with a wrong mean distance, how many neighbours it loses."""
    xyz = np.asarray(xyz, F32)
    want = k + 1
    wrong = lost = 0
    for s in range(0, len(xyz), 256):
        P = xyz[s:s + 256, None, :]
        d2 = fdist2(P, xyz[None])
        acc = accept(d2, h, "knn")
        fnd = acc & found("old", P, xyz[None], h, lo, n)
        lost += int((acc & ~fnd).sum())
        for i in range(len(d2)):
            if fnd[i].sum() < want:
                continue                                   # undecided: the next level takes it
            t = np.sort(d2[i][acc[i]])[:want]
            f = np.sort(d2[i][fnd[i]])[:want]
            wrong += int(np.sum(np.sqrt(t).astype(F64)) != np.sum(np.sqrt(f).astype(F64)))
    return dict(wrong=wrong, lost=lost)
