"""A second, independent statement of the isdelete branch of CCloudOptimization::run (CCloudOptimization.cpp:152-346), written from
DESIGN 9 f6's rules as the reference writes them: one point at a time, real per-pixel bucket lists filled in point order, pairs /
rows / columns visited in nested loops, and for three or more candidates the reference's repeated first-maximum selection
(:282-296: strict '<' from 0, the chosen distance set to 0) -- no sort anywhere.  Scalars are np.float32 where the reference
computes in float, reduced as (a0 b0 + a1 b1) + a2 b2; ROUND is int(float64(q) + 0.5).  What the reference leaves undefined is
defined as DESIGN 9 f6 lists it.  CurrentValue alone is shared with tests/dedup_restatement.py (current_value: the oracle's
Armadillo-order primitives); tests/test_dedup_edges_cpu.py holds it to a plain numpy correlation.

dedup(xyz, normals, views, trace=None) takes dedup_restatement's view dicts.  trace, when a dict, receives
  "cv":      {(pair, X, Y): CurrentValue} for every pixel the value was read at,
  "buckets": [(pair, X, Y, [point indices])] for every visited bucket, in visiting order,
  "order":   {(pair, X, Y): [bucket positions, farthest first]} for buckets of three or more,
  "owner":   [pair or -1 per point] (-1: s1 or s2), "values": [[best-pair value per pair] per point].
"""
from __future__ import annotations

import numpy as np

from dedup_restatement import current_value

F = np.float32
FLT_MIN = F(1.17549435e-38)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def round_(q):
    """ROUND (SharedInclude.h:48); None where the reference is undefined (non-finite, outside int)."""
    v = float(q) + 0.5
    if not (v > -2147483649.0 and v < 2147483648.0):
        return None
    return int(v)


def project(R, T, p):
    q = [dot3(R[r], p) + T[r] for r in range(3)]
    x, y = round_(q[0] / q[2]), round_(q[1] / q[2])
    return None if x is None or y is None else (x, y)


def _rt(P):
    P = np.asarray(P, np.float64).reshape(3, 4)
    return [[F(P[r, k]) for k in range(3)] for r in range(3)], [F(P[r, 3]) for r in range(3)]


def farthest_first(dist):
    """:282-296 on a list of distances: bucket positions, farthest first; candidates whose distance is not > 0 (0 or NaN; the
    reference indexes current_dist[-1] there) follow in bucket order.  Python floats hold the float32 values exactly."""
    cur = [float(d) for d in dist]
    order = []
    for _ in range(len(cur)):
        mx, mi = 0.0, -1
        for k in range(len(cur)):
            if mx < cur[k]:
                mx, mi = cur[k], k
        if mi < 0:
            break
        cur[mi] = 0.0
        order.append(mi)
    return order + [k for k in range(len(dist)) if not float(dist[k]) > 0.0]


def dedup(xyz, normals, views, trace=None):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    nrm = np.asarray(normals, np.float32).reshape(n, -1)[:, :3] if n else np.zeros((0, 3), np.float32)
    st = dict(s1=0, s2=0, count0=0, visited=0)
    tr = trace if trace is not None else {}
    tr.update(cv={}, buckets=[], order={}, owner=[-1] * n, values=[None] * n)
    cams = []
    for v in views:
        YL, YR, XL, XR, w, h = [int(t) for t in v["bound"]]
        cams.append(dict(L=_rt(v["P"][0]), R=_rt(v["P"][1]), C=[F(t) for t in np.asarray(v["C"], np.float32).ravel()[:3]],
                         YL=YL, YR=YR, XL=XL, XR=XR, w=w, h=h, m0=np.asarray(v["mask"][0]), m1=np.asarray(v["mask"][1]),
                         bucket=[[[] for _ in range(w)] for _ in range(h)] if w > 0 and h > 0 else None))
    out = []
    with np.errstate(all="ignore"):
        # :160-192
        for j in range(n):
            p, nv = xyz[j], nrm[j]
            best, b, vals = FLT_MIN, 0, []
            for i, c in enumerate(cams):
                cd = [c["C"][k] - p[k] for k in range(3)]
                val = dot3(nv, cd) / np.sqrt(dot3(cd, cd))
                vals.append(val)
                if best < val:
                    best, b = val, i
            tr["values"][j] = vals
            c = cams[b]
            xy = project(c["L"][0], c["L"][1], p)
            if xy is None or c["bucket"] is None:
                st["s1"] += 1
                continue
            x, y = xy[0] - c["XL"], xy[1] - c["YL"]
            if x < 0 or x >= c["w"] or y < 0 or y >= c["h"]:
                st["s1"] += 1
                continue
            if c["m0"][y + c["YL"], x + c["XL"]] == 0:
                st["s2"] += 1
                continue
            c["bucket"][y][x].append(j)
            tr["owner"][j] = b
        # :203-337
        for i, c in enumerate(cams):
            if c["bucket"] is None:
                continue
            H1, W1 = c["m1"].shape

            def right_ok(j):
                xy = project(c["R"][0], c["R"][1], xyz[j])
                if xy is not None and 0 <= xy[0] < W1 and 0 <= xy[1] < H1 and c["m1"][xy[1], xy[0]] == 255:
                    return True
                st["count0"] += 1
                return False

            for Y in range(c["YL"], c["YR"] + 1):
                for X in range(c["XL"], c["XR"] + 1):
                    if c["m0"][Y, X] != 255:
                        continue
                    bk = c["bucket"][Y - c["YL"]][X - c["XL"]]
                    size = len(bk)
                    if size == 0:
                        continue
                    st["visited"] += 1
                    tr["buckets"].append((i, X, Y, list(bk)))

                    def value():
                        if (i, X, Y) not in tr["cv"]:
                            tr["cv"][(i, X, Y)] = current_value(views[i], X, Y)
                        return tr["cv"][(i, X, Y)]

                    if size == 1:
                        out.append(bk[0])
                    elif size == 2:
                        if dot3(nrm[bk[0]], nrm[bk[1]]) < 0:
                            out += [bk[0], bk[1]]
                        else:
                            ti, mx = -1, -1.0
                            for k in range(2):
                                if not right_ok(bk[k]):
                                    continue
                                if value() > mx:
                                    ti, mx = k, value()
                            if ti >= 0:
                                out.append(bk[ti])
                    else:
                        dist, direct = [], []
                        for l in range(size):
                            d = [xyz[bk[l]][k] - c["C"][k] for k in range(3)]
                            dist.append(np.sqrt(dot3(d, d)))
                            direct.append(bool(dot3(nrm[bk[l]], d) < 0))
                        srt = farthest_first(dist)
                        tr["order"][(i, X, Y)] = srt
                        last = 0
                        for l in range(1, size):
                            if direct[srt[last]] == direct[srt[l]] and l != size - 1:
                                continue
                            ti = last
                            if last + 1 < l:
                                mx = -1.0
                                for k in range(last, l):
                                    if not right_ok(bk[srt[k]]):
                                        continue
                                    if value() > mx:
                                        ti, mx = k, value()
                            out.append(bk[srt[ti]])
                            last = l
    return np.asarray(out, np.int32), st
