"""numpy float64 restatement of the moving-least-squares step (CCloudOptimization::run, CloudOptimization/CCloudOptimization.cpp:
348-389): PCL 1.7.2's MovingLeastSquares::computeMLSPointNormal for upsampling NONE, as csrc/k_mls.hip states it, plus the normal
flip of :378-385.  Test infrastructure only (oracle/ stays as it is); no scipy.

Per finite input point p:
  neighbours: the finite q with float32 (dx*dx + dy*dy) + dz*dz < r*r (p included); fewer than 3: no output;
  plane: double centroid c, de-meaned covariance sum (q - c)(q - c)^T, eigen33 (PCL's, as cloud_grid.h's pcl_plane_from_cov):
    normal n of the smallest eigenvalue, curvature |lambda / trace|; pt = p - (n.p - n.c) n;
  polynomial fit (order > 0, at least (order + 1)(order + 2) / 2 neighbours): v = n.unitOrthogonal() (Eigen), u = n x v,
    e = q - pt, w = exp(-(e.e) / r^2), terms uc^i vc^j in PCL's order, (P W P^T) c = P W f by Cholesky (a pivot that is not
    positive: no fit); c[0] finite: pt += c[0] n, normal = n - (c[order + 1] u + c[1] v) (not renormalised).
Neighbours are found through an x-sorted slab (searchsorted on x +- r), a block of nearby queries at a time.
"""
from __future__ import annotations

import numpy as np


def plane_from_cov(cov, census=None):
    """PCL's eigen33 (smallest eigenvalue, its unit vector) + curvature |lambda / trace| on a batch [B,3,3] of covariances.
    census (a dict, optional) receives the branch each covariance took: c0_small (computeRoots2 because |c0| < eps), fallback (the
    trigonometric roots with r0 <= 0, then computeRoots2), r0 (the smallest trigonometric root), pick (1, 2, 3: which cross product
    won) and tie (won on an equal length)."""
    cov = np.asarray(cov, np.float64)
    B = len(cov)
    c = cov.reshape(B, 9)
    with np.errstate(all="ignore"):
        scale = np.fmax(np.fmax.reduce(np.abs(c), axis=1), 0.0)
        scale = np.where(scale <= 2.2250738585072014e-308, 1.0, scale)
        m = c / scale[:, None]
        m0, m1, m2, m3, m4, m5, m6, m7, m8 = (m[:, i] for i in range(9))
        c0 = m0 * m4 * m8 + 2.0 * m1 * m2 * m5 - m0 * m5 * m5 - m4 * m2 * m2 - m8 * m1 * m1
        c1 = m0 * m4 - m1 * m1 + m0 * m8 - m2 * m2 + m4 * m8 - m5 * m5
        c2 = m0 + m4 + m8

        def roots2_low(b, cc):      # computeRoots2: roots (0, (b - sd) / 2, (b + sd) / 2): the smallest is 0
            return np.zeros_like(b)

        s_inv3, s_sqrt3 = 1.0 / 3.0, np.sqrt(3.0)
        c2_over_3 = c2 * s_inv3
        a_over_3 = (c1 - c2 * c2_over_3) * s_inv3
        a_over_3 = np.where(a_over_3 > 0.0, 0.0, a_over_3)
        half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1))
        q = half_b * half_b + a_over_3 * a_over_3 * a_over_3
        q = np.where(q > 0.0, 0.0, q)
        rho = np.sqrt(-a_over_3)
        theta = np.arctan2(np.sqrt(-q), half_b) * s_inv3
        ct, st = np.cos(theta), np.sin(theta)
        r0 = c2_over_3 + 2.0 * rho * ct
        r1 = c2_over_3 - rho * (ct + s_sqrt3 * st)
        r2 = c2_over_3 - rho * (ct - s_sqrt3 * st)
        # the kernel's sorting network: (r0, r1), then (r1, r2) and, after that swap, (r0, r1) again
        sw = r0 >= r1
        r0, r1 = np.where(sw, r1, r0), np.where(sw, r0, r1)
        sw = r1 >= r2
        r1, r2 = np.where(sw, r2, r1), np.where(sw, r1, r2)
        sw2 = sw & (r0 >= r1)
        r0, r1 = np.where(sw2, r1, r0), np.where(sw2, r0, r1)
        low = np.where(r0 <= 0.0, roots2_low(c2, c1), r0)
        low = np.where(np.abs(c0) < 2.220446049250313e-16, roots2_low(c2, c1), low)
        ev = low * scale
        d0, d4, d8 = m0 - low, m4 - low, m8 - low
        v1 = np.stack([m1 * m5 - m2 * d4, m2 * m3 - d0 * m5, d0 * d4 - m1 * m3], 1)
        v2 = np.stack([m1 * d8 - m2 * m7, m2 * m6 - d0 * d8, d0 * m7 - m1 * m6], 1)
        v3 = np.stack([d4 * d8 - m5 * m7, m5 * m6 - m3 * d8, m3 * m7 - d4 * m6], 1)
        l1 = v1[:, 0] * v1[:, 0] + v1[:, 1] * v1[:, 1] + v1[:, 2] * v1[:, 2]
        l2 = v2[:, 0] * v2[:, 0] + v2[:, 1] * v2[:, 1] + v2[:, 2] * v2[:, 2]
        l3 = v3[:, 0] * v3[:, 0] + v3[:, 1] * v3[:, 1] + v3[:, 2] * v3[:, 2]
        pick1 = (l1 >= l2) & (l1 >= l3)
        pick2 = ~pick1 & (l2 >= l1) & (l2 >= l3)
        v = np.where(pick1[:, None], v1, np.where(pick2[:, None], v2, v3))
        l = np.where(pick1, l1, np.where(pick2, l2, l3))
        n = v / np.sqrt(l)[:, None]
        if census is not None:
            c0_small = np.abs(c0) < 2.220446049250313e-16
            census.update(c0_small=c0_small, fallback=~c0_small & (r0 <= 0.0), r0=r0, pick=np.where(pick1, 1, np.where(pick2, 2, 3)),
                          tie=(pick1 & ((l1 == l2) | (l1 == l3))) | (pick2 & (l2 == l3)))
        tr = cov[:, 0, 0] + cov[:, 1, 1] + cov[:, 2, 2]
        curv = np.where(tr != 0.0, np.abs(ev / tr), 0.0)
    return n, curv


def unit_orthogonal(n):
    """Eigen's MatrixBase::unitOrthogonal for 3-vectors (isMuchSmallerThan with double precision 1e-12), batch [B,3]."""
    n = np.asarray(n, np.float64)
    a = (np.abs(n[:, 0]) > np.abs(n[:, 2]) * 1e-12) | (np.abs(n[:, 1]) > np.abs(n[:, 2]) * 1e-12)
    with np.errstate(all="ignore"):
        inv1 = 1.0 / np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1])
        inv2 = 1.0 / np.sqrt(n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        return np.stack([np.where(a, -n[:, 1] * inv1, 0.0), np.where(a, n[:, 0] * inv1, -n[:, 2] * inv2),
                         np.where(a, 0.0, n[:, 1] * inv2)], 1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _llt_solve(A, b):
    """Cholesky (A = L L^T) and the two triangular solves, batch; ok = every pivot positive."""
    B, N = b.shape
    L = np.zeros_like(A)
    ok = np.ones(B, bool)
    with np.errstate(all="ignore"):
        for k in range(N):
            x = A[:, k, k].copy()
            for m in range(k):
                x -= L[:, k, m] * L[:, k, m]
            ok &= x > 0.0
            dkk = np.sqrt(x)
            L[:, k, k] = dkk
            for r in range(k + 1, N):
                s = A[:, r, k].copy()
                for m in range(k):
                    s -= L[:, r, m] * L[:, k, m]
                L[:, r, k] = s / dkk
        c = np.zeros_like(b)
        for k in range(N):
            s = b[:, k].copy()
            for m in range(k):
                s -= L[:, k, m] * c[:, m]
            c[:, k] = s / L[:, k, k]
        for k in range(N - 1, -1, -1):
            s = c[:, k].copy()
            for m in range(k + 1, N):
                s -= L[:, m, k] * c[:, m]
            c[:, k] = s / L[:, k, k]
    return c, ok


def _terms(uc, vc, order):
    out = []
    u_pow = np.ones_like(uc)
    for ui in range(order + 1):
        v_pow = np.ones_like(vc)
        for vi in range(order - ui + 1):
            out.append(u_pow * v_pow)
            v_pow = v_pow * vc
        u_pow = u_pow * uc
    return np.stack(out, -1)


def mls(xyz, radius, orders=(1,), ref_normals=None, queries=None, block=256, census=None):
    """The MLS output of the queried input points (default: all) for each polynomial order in `orders`.

    Returns {order: (emit bool [q], xyz float32 [q,3], normals float32 [q,4] = nx, ny, nz, curvature)} for the queries in the
    order given (their input indices); rows where emit is False carry nothing.  ref_normals ([n,>=3]): the flip of :378-385.
    census (a dict, optional) receives per query: cnt, plane_from_cov's branches, uo_form (1, 2: unitOrthogonal's form) and, per order
    o > 0, ("pivots_ok", o) (every Cholesky pivot positive) and ("c0_finite", o)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n_all = len(xyz)
    q_idx = np.arange(n_all) if queries is None else np.asarray(queries, np.int64).ravel()
    fin = np.isfinite(xyz).all(1)
    idx_f = np.nonzero(fin)[0]
    srt = np.argsort(xyz[idx_f, 0], kind="stable")
    Xs, Is = xyz[idx_f][srt], idx_f[srt]
    xs = Xs[:, 0]
    r = float(radius)
    r2f = np.float32(r * r)
    gauss = r * r
    res = {o: (np.zeros(len(q_idx), bool), np.full((len(q_idx), 3), np.nan, np.float32), np.full((len(q_idx), 4), np.nan, np.float32))
           for o in orders}
    live = np.nonzero(fin[q_idx])[0]                     # non-finite points: nobody's neighbour, no output
    if len(live) == 0:
        return res
    qp = xyz[q_idx[live]]
    # blocks of nearby queries: sorted by (column of width r in x, y), cut at `block` queries or 4 r of y
    key = np.lexsort((qp[:, 1], np.floor(qp[:, 0] / r)))
    col = np.floor(qp[key, 0] / r)
    ys = qp[key, 1]
    starts = [0]
    for t in range(1, len(key)):
        s0 = starts[-1]
        if t - s0 >= block or col[t] != col[s0] or ys[t] - ys[s0] > 4.0 * r:
            starts.append(t)
    starts.append(len(key))
    ref = None if ref_normals is None else np.asarray(ref_normals, np.float32).reshape(n_all, -1)[:, :3]
    pad = r * 1.001 + 1e-3
    for b0, b1 in zip(starts[:-1], starts[1:]):
        rows = live[key[b0:b1]]                          # positions in q_idx
        Q = xyz[q_idx[rows]]
        lo = np.searchsorted(xs, Q[:, 0].min() - pad, "left")
        hi = np.searchsorted(xs, Q[:, 0].max() + pad, "right")
        Cx, Ci = Xs[lo:hi], Is[lo:hi]
        box = ((Cx[:, 1] >= Q[:, 1].min() - pad) & (Cx[:, 1] <= Q[:, 1].max() + pad) &
               (Cx[:, 2] >= Q[:, 2].min() - pad) & (Cx[:, 2] <= Q[:, 2].max() + pad))
        Cc = Cx[box]
        d = [Q[:, None, a] - Cc[None, :, a] for a in range(3)]          # float32, as the kernel
        M = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < r2f
        used = M.any(0)                                                  # candidates some query of the block has as neighbour
        M, Cc = M[:, used], Cc[used]
        cnt = M.sum(1)
        Mf = M.astype(np.float64)
        C64 = Cc.astype(np.float64)
        with np.errstate(all="ignore"):
            cen = (Mf @ C64) / cnt[:, None]
            D = C64[None] - cen[:, None]
            cov = np.matmul((D * Mf[..., None]).transpose(0, 2, 1), D)
            cen_b = None if census is None else {}
            nrm, curv = plane_from_cov(cov, cen_b)
            if census is not None:
                cen_b["cnt"] = cnt
                cen_b["uo_form"] = np.where((np.abs(nrm[:, 0]) > np.abs(nrm[:, 2]) * 1e-12) | (np.abs(nrm[:, 1]) > np.abs(nrm[:, 2]) * 1e-12), 1, 2)
            dd = -_dot3(nrm, cen)
            p64 = Q.astype(np.float64)
            dist = ((p64[:, 0] * nrm[:, 0] + p64[:, 1] * nrm[:, 1]) + p64[:, 2] * nrm[:, 2]) + dd
            pt = p64 - dist[:, None] * nrm
        emit = cnt >= 3
        for o in orders:
            pto, no = pt, nrm
            if o > 0:
                nc = (o + 1) * (o + 2) // 2
                with np.errstate(all="ignore"):
                    v = unit_orthogonal(nrm)
                    u = _cross(nrm, v)
                    E = C64[None] - pt[:, None]
                    w = np.exp(-_dot3(E, E) / gauss) * Mf
                    uc, vc, f = _dot3(E, u[:, None]), _dot3(E, v[:, None]), _dot3(E, nrm[:, None])
                    P = _terms(uc, vc, o)
                    PW = (P * w[..., None]).transpose(0, 2, 1)
                    A = np.matmul(PW, P)
                    bb = np.matmul(PW, f[..., None])[..., 0]
                    c, ok = _llt_solve(A, bb)
                    fit = (cnt >= nc) & ok & np.isfinite(c[:, 0])
                    if census is not None:
                        cen_b[("pivots_ok", o)], cen_b[("c0_finite", o)] = ok, np.isfinite(c[:, 0])
                    pto = np.where(fit[:, None], pt + c[:, :1] * nrm, pt)
                    no = np.where(fit[:, None], nrm - (c[:, o + 1:o + 2] * u + c[:, 1:2] * v), nrm)
            fn = no.astype(np.float32)
            if ref is not None:
                rn = ref[q_idx[rows]]
                flip = ((fn[:, 0] * rn[:, 0] + fn[:, 1] * rn[:, 1]) + fn[:, 2] * rn[:, 2]) < np.float32(0)
                fn = np.where(flip[:, None], -fn, fn)
            e_, x_, n_ = res[o]
            e_[rows] = emit
            x_[rows] = np.where(emit[:, None], pto.astype(np.float32), np.nan)
            n_[rows, :3] = np.where(emit[:, None], fn, np.nan)
            n_[rows, 3] = np.where(emit, curv.astype(np.float32), np.nan)
        if census is not None:
            for k, val in cen_b.items():
                census.setdefault(k, np.zeros(len(q_idx), np.asarray(val).dtype))[rows] = val
    return res


def mls_cloud(xyz, radius, order=1, ref_normals=None):
    """The whole cloud as rsm_mls_cloud returns it: (xyz float32 [m,3], normals float32 [m,4], src_index int32 [m])."""
    emit, x, nrm = mls(xyz, radius, (order,), ref_normals)[order]
    idx = np.nonzero(emit)[0]
    return x[idx], nrm[idx], idx.astype(np.int32)
