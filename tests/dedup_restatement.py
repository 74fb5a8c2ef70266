"""numpy restatement of the isdelete branch of CCloudOptimization::run (CloudOptimization/CCloudOptimization.cpp:152-346): the
multi-view duplicate deletion that csrc/k_dedup.hip runs on the GPU.  Same rules, same definitions of what the reference leaves
undefined; float32 where the reference computes in float (numpy float32 arithmetic is IEEE single, no FMA), the NCC
in fp64 through the CPU oracle's Armadillo-order primitives (oracle.arma_mean / arma_norm2 / arma_dot).

A view is a dict: P = [P0, P1] (3x4 fp64, cam[i][k].P), C (cam[i][0].CamCenter), bound (YL, YR, XL, XR, width, height),
image = [BGR, BGR], mask = [u8, u8].  views_from_cams turns m_ImageData.cam into that form.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as orc

FLT_MIN = np.float32(1.17549435e-38)
R_WIN = 2   # MatchBlockRadius of the branch (:199)


def _dot3(a, b):
    """The Eigen 3-vector reduction order chosen for dots, squared norms and the rows of R p (k_dedup.hip: dd_dot3)."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _round(q):
    """ROUND (SharedInclude.h:48) of float quotients: (ok, int64); not ok where the reference is undefined."""
    v = np.asarray(q, np.float32).astype(np.float64) + 0.5
    ok = (v > -2147483649.0) & (v < 2147483648.0)
    r = np.zeros(v.shape, np.int64)
    r[ok] = np.trunc(v[ok]).astype(np.int64)
    return ok, r


def _RT(P):
    P = np.asarray(P, np.float64).reshape(3, 4)
    return P[:, :3].astype(np.float32), P[:, 3].astype(np.float32)


def _project(R, T, p):
    p = np.asarray(p, np.float32).reshape(-1, 3)
    q = [_dot3(R[r][None, :], p) + T[r] for r in range(3)]
    with np.errstate(all="ignore"):
        okx, x = _round(q[0] / q[2])
        oky, y = _round(q[1] / q[2])
    return okx & oky, x, y


def views_from_cams(cams):
    return [dict(P=[c[0].P, c[1].P], C=c[0].CamCenter, bound=tuple(c[0].bound), image=[c[0].image, c[1].image],
                 mask=[c[0].mask, c[1].mask]) for c in cams]


def _wvec(img, X, Y):
    """CManageData::WindowToVec, cv::Mat overload (CManageData.h:45-59): rows outer, bytes inner, de-meaned, its norm (0 -> 1)."""
    u = np.ascontiguousarray(img[Y - R_WIN:Y + R_WIN + 1, X - R_WIN:X + R_WIN + 1, :]).reshape(-1).astype(np.float64)
    u = u - orc.arma_mean(u)
    nu = orc.arma_norm2(u)
    return u, (1.0 if nu == 0 else nu)


def current_value(view, X, Y):
    """CurrentValue at the left pixel (X, Y): both windows at (X - 2, Y - 2) (:241, :254 / :310, :322)."""
    uL, nL = _wvec(view["image"][0], X, Y)
    uR, nR = _wvec(view["image"][1], X, Y)
    return orc.arma_dot(uL, uR) / (nR * nL)


def dedup(xyz, normals, views):
    """Returns (indicesptr int32, dict(s1, s2, count0, visited))."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    st = dict(s1=0, s2=0, count0=0, visited=0)
    if n == 0:      # (before the normals: an empty array has no row length to infer)
        return np.zeros(0, np.int32), st
    nrm = np.asarray(normals, np.float32).reshape(n, -1)[:, :3].copy()
    RT = [(_RT(v["P"][0]), _RT(v["P"][1])) for v in views]
    C = [np.asarray(v["C"], np.float32).ravel()[:3] for v in views]
    # loop 1 (:160-192): best pair, projection, buckets
    best = np.full(n, FLT_MIN, np.float32)
    b = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for i in range(len(views)):
            cd = C[i][None, :] - xyz
            val = _dot3(nrm, cd) / np.sqrt(_dot3(cd, cd))
            upd = best < val
            best[upd] = val[upd]
            b[upd] = i
    key = np.full(n, -1, np.int64)
    base = 0
    for i, v in enumerate(views):
        YL, YR, XL, XR, w, h = [int(t) for t in v["bound"]]
        empty = w <= 0 or h <= 0
        sel = np.nonzero(b == i)[0]
        ok, X, Y = _project(*RT[i][0], xyz[sel])
        x, y = X - XL, Y - YL
        inb = ok & (x >= 0) & (x < w) & (y >= 0) & (y < h) if not empty else np.zeros(len(sel), bool)
        st["s1"] += int((~inb).sum())
        m0 = np.asarray(v["mask"][0])
        on = np.zeros(len(sel), bool)
        on[inb] = m0[Y[inb], X[inb]] != 0
        st["s2"] += int((inb & ~on).sum())
        key[sel[on]] = base + y[on] * w + x[on]
        if not empty:
            base += w * h
    # loop 2 (:203-337): buckets in (pair, y, x) order, members ascending
    val = np.nonzero(key >= 0)[0]
    order = val[np.argsort(key[val], kind="stable")]
    ks = key[order]
    starts = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0] if len(ks) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(ks)].astype(np.int64)
    bases, base = [], 0
    for v in views:
        w, h = int(v["bound"][4]), int(v["bound"][5])
        bases.append(base if (w > 0 and h > 0) else None)
        if w > 0 and h > 0:
            base += w * h
    out = []
    for s, e in zip(starts, ends):
        k = int(ks[s])
        i = max(t for t in range(len(views)) if bases[t] is not None and bases[t] <= k)
        v = views[i]
        YL, YR, XL, XR, w, h = [int(t) for t in v["bound"]]
        X, Y = (k - bases[i]) % w + XL, (k - bases[i]) // w + YL
        if np.asarray(v["mask"][0])[Y, X] != 255:
            continue
        st["visited"] += 1
        bucket = [int(t) for t in order[s:e]]
        cv = []   # CurrentValue, once per bucket (it does not depend on the candidate)

        def passes(j):
            ok, x1, y1 = _project(*RT[i][1], xyz[j])
            m1 = np.asarray(v["mask"][1])
            good = bool(ok[0]) and 0 <= x1[0] < m1.shape[1] and 0 <= y1[0] < m1.shape[0] and m1[y1[0], x1[0]] == 255
            if not good:
                st["count0"] += 1
            return good

        def value():
            if not cv:
                cv.append(current_value(v, X, Y))
            return cv[0]

        if len(bucket) == 1:
            out.append(bucket[0])
        elif len(bucket) == 2:
            if _dot3(nrm[bucket[0]], nrm[bucket[1]]) < 0:
                out += bucket
            else:
                ti, mx = -1, -1.0
                for t in range(2):
                    if not passes(bucket[t]):
                        continue
                    if value() > mx:
                        ti, mx = t, value()
                if ti >= 0:
                    out.append(bucket[ti])
        else:
            P = xyz[bucket]
            direct = P - C[i][None, :]
            d = np.sqrt(_dot3(direct, direct))
            dirs = _dot3(nrm[bucket], direct) < 0
            good = [l for l in range(len(bucket)) if d[l] > 0]
            srt = sorted(good, key=lambda l: -float(d[l])) + [l for l in range(len(bucket)) if not d[l] > 0]
            last = 0
            for l in range(1, len(bucket)):
                if dirs[srt[last]] == dirs[srt[l]] and l != len(bucket) - 1:
                    continue
                ti = last
                if last + 1 < l:
                    mx = -1.0
                    for t in range(last, l):
                        if not passes(bucket[srt[t]]):
                            continue
                        if value() > mx:
                            ti, mx = t, value()
                out.append(bucket[srt[ti]])
                last = l
    return np.asarray(out, np.int32), st


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def ray_view(W=40, H=30, t=-4.0, seed=0, bound=None, C=(0.0, 0.0, 0.0)):
    """A hand-checkable pair: P0 = [I | 0] (a point (x z, y z, z) lands on pixel (x, y) at every depth z > 0), P1 = [I | (t, 0, 0)],
    random textures, masks all 255, bound 3 px inside the image."""
    rng = np.random.default_rng(seed)
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    P1 = np.hstack([np.eye(3), np.array([[t], [0.0], [0.0]])])
    img = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)]
    msk = [np.full((H, W), 255, np.uint8) for _ in range(2)]
    if bound is None:
        bound = (3, H - 4, 3, W - 4, W - 6, H - 6)
    return dict(P=[P0, P1], C=np.asarray(C, np.float32), bound=bound, image=img, mask=msk)


def on_ray(x, y, z):
    return [x * z, y * z, z]


def _look_at(C, target=(0.0, 0.0, 0.0)):
    f = np.asarray(target, np.float64) - C
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0])
    r /= np.linalg.norm(r)
    u = np.cross(f, r)
    return np.stack([r, u, f])      # rows: camera x, y, z in world coordinates (x_cam = R (X - C))


def random_scene(seed, n, n_pairs, W=256, H=192, f=300.0, empty_pair=False):
    """Pairs looking at a sphere of radius 100 from distance 500, rectified-style right views 40 units along the camera x; points on
    the sphere with noisy outward normals, a share of them layered along their pair's ray (thick surfaces), exact duplicates, some
    flipped and a few NaN normals; masks with 0 and 1..254 areas."""
    rng = np.random.default_rng(seed)
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    views = []
    for i in range(n_pairs):
        th = 2 * np.pi * i / max(n_pairs, 1) * 0.35
        Cw = np.array([500 * np.sin(th), 30.0 * (i % 2), -500 * np.cos(th)])
        R = _look_at(Cw)
        P0 = K @ np.hstack([R, (-R @ Cw)[:, None]])
        C1 = Cw + 40.0 * R[0]
        P1 = K @ np.hstack([R, (-R @ C1)[:, None]])
        img = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)]
        msk = []
        for _ in range(2):
            m = np.full((H, W), 255, np.uint8)
            for _ in range(6):
                y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
                m[y0:y0 + rng.integers(4, 30), x0:x0 + rng.integers(4, 30)] = rng.choice([0, 0, 17, 254])
            msk.append(m)
        YL, XL = int(rng.integers(2, 12)), int(rng.integers(2, 12))
        YR, XR = H - 3 - int(rng.integers(0, 10)), W - 3 - int(rng.integers(0, 10))
        bound = (YL, YR, XL, XR, XR - XL + 1, YR - YL + 1)
        if empty_pair and i == n_pairs - 1:
            bound = (H - 3, 2, W - 3, 2, 2 - (W - 3) + 1, 2 - (H - 3) + 1)
        views.append(dict(P=[P0, P1], C=Cw.astype(np.float32), bound=bound, image=img, mask=msk))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = -np.abs(d[:, 2])                      # the hemisphere the rig sees
    p = 100.0 * d
    nrm = d + 0.3 * rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    # thick layers: copies pushed along the view ray of a random pair, with own normals
    k = n // 3
    src = rng.integers(0, n, k)
    cam = np.stack([views[j]["C"] for j in rng.integers(0, n_pairs, k)]).astype(np.float64)
    ray = p[src] - cam
    ray /= np.linalg.norm(ray, axis=1, keepdims=True)
    p[:k] = p[src] + ray * rng.uniform(-3, 3, (k, 1))
    nrm[:k] = nrm[src] * np.where(rng.random((k, 1)) < 0.3, -1.0, 1.0)
    dup = rng.integers(0, n, n // 50)
    p[rng.integers(0, n, n // 50)] = p[dup]
    nrm[rng.integers(0, n, n // 200)] = np.nan
    n4 = np.zeros((n, 4), np.float32)
    n4[:, :3] = nrm
    n4[:, 3] = rng.random(n)
    return p.astype(np.float32), n4, views
