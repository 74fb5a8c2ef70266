"""Scenes for the duplicate deletion (csrc/k_dedup.hip) built to sit on its decisions: CurrentValue within an ulp of
-1, every small bucket pattern, buckets on the wave / block boundaries of the sorted array, 2^k key totals, pairs of unequal image
size with empty ones among them, best-pair values that tie or differ by one float ulp, and ROUND at the halves.  Each fixture
returns (xyz float32 [n,3], normals float32 [n,4], views) in tests/dedup_restatement.py's form; FIXTURES lists every variant.
What a fixture claims to reach is asserted in tests/test_dedup_edges_cpu.py from the two CPU statements, never from the kernel.

All left views are P0 = [I | 0]: the point (x z, y z, z) lands on pixel (x, y) at every depth z (near_ties uses an orthographic P0).
The right views are functions of depth alone, e.g. [[0,0,1,0],[0,0,0,b],[0,0,0,1]] sends depth z to pixel (ROUND(z), b), so a mask
row that alternates 255 / 0 lets each candidate's right-mask outcome be chosen by its depth's parity, whatever its distance rank.
CamCenter is a field of its own in the view (the reference reads it from a file), so it need not be P0's centre.

Out of scope here: the 64-bit key instantiation (it needs a key total of 2^32 or more, so masks of 4 GB; no input reaches it in
seconds and no hook is added for it), the open Eigen reduction-order question (it stays in dd_dot3 / _dot3), and the bounds the
entry refuses (test_gpu_dedup.py::test_invalid_arguments has them).
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

TOWARD = (0.0, 0.0, -1.0, 0.0)
AWAY = (0.0, 0.0, 1.0, 0.0)
P0_RAY = np.hstack([np.eye(3), np.zeros((3, 1))])


def on_ray(x, y, z):
    z = np.float32(z)
    return [np.float32(x) * z, np.float32(y) * z, z]


def depth_P1(row, a=1.0, t=0.0, to_row=False):
    """Right view (ROUND(a z + t), row), or (row, ROUND(a z + t)) with to_row."""
    moving, fixed = [0.0, 0.0, a, t], [0.0, 0.0, 0.0, float(row)]
    return np.array([fixed, moving, [0, 0, 0, 1.0]] if to_row else [moving, fixed, [0, 0, 0, 1.0]], np.float64)


def inner_bound(W, H, m=2):
    return (m, H - 1 - m, m, W - 1 - m, W - 2 * m, H - 2 * m)


def empty_bound(W, H):
    return (H - 3, 2, W - 3, 2, 2 - (W - 3) + 1, 2 - (H - 3) + 1)


def view(W, H, seed, anti, bound=None, C=(0.0, 0.0, 0.0), P0=P0_RAY, P1=None, mask1=None):
    """Random left image; the right image is 255 - left (anti: vecR = -vecL up to rounding, CurrentValue within an ulp of -1) or
    random too; masks 255 unless given."""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    right = (255 - left).astype(np.uint8) if anti else rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    m1 = np.full((H, W), 255, np.uint8) if mask1 is None else mask1
    return dict(P=[np.array(P0, np.float64), depth_P1(0) if P1 is None else P1], C=np.asarray(C, np.float32),
                bound=inner_bound(W, H) if bound is None else bound, image=[left, right], mask=[np.full((H, W), 255, np.uint8), m1])


def alternating_mask1(W, H, row):
    """255 on the even columns of one row, 0 elsewhere."""
    m = np.zeros((H, W), np.uint8)
    m[row, 0::2] = 255
    return m


def toward(p, C):
    d = np.asarray(C, np.float64) - np.asarray(p, np.float64)
    d /= np.linalg.norm(d)
    return [d[0], d[1], d[2], 0.0]


def _pack(pts, nrm):
    if not pts:
        return np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32)
    return np.asarray(pts, np.float32).reshape(-1, 3), np.asarray(nrm, np.float32).reshape(-1, 4)


def _interleave(groups, seed):
    """Point order for a list of buckets (each a list of (point, normal)): every bucket keeps its members' order, and members of one
    bucket lie far apart in the cloud (all first members in a shuffled order, then all second members, ...)."""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for pos in range(max([len(g) for g in groups] + [0])):
        for gi in rng.permutation(len(groups)):
            if pos < len(groups[gi]):
                pts.append(groups[gi][pos][0])
                nrm.append(groups[gi][pos][1])
    return _pack(pts, nrm)


# ---- minus_one --------------------------------------------------------------------------------------------------------------------
MINUS_ONE_FLAT = (slice(4, 13), slice(4, 13))       # rows, columns: both images flat (norm 0: CurrentValue 0)
MINUS_ONE_RANDOM = (slice(16, 26), slice(24, 36))   # the right image random here


def minus_one(seed=0):
    """Two pairs over the same 40x30 images, right = 255 - left.  Pair 0 (CamCenter 0): every bound pixel holds two same-direction
    points at depths 10 and 12, both passing the right mask: the first is kept iff CurrentValue > -1.  Pair 1 (CamCenter
    (0, 0, -1000)): every bound pixel holds three points of one direction at depths 10, 8, 11; the farthest (11) misses the right
    mask and the next (10) passes, so depth 10 is kept iff CurrentValue > -1 and the farthest otherwise."""
    W, H = 40, 30
    m1 = alternating_mask1(W, H, 5)
    a = view(W, H, seed, True, P1=depth_P1(5), mask1=m1)
    a["image"][0][MINUS_ONE_FLAT], a["image"][1][MINUS_ONE_FLAT] = 90, 165
    a["image"][1][MINUS_ONE_RANDOM] = np.random.default_rng(seed + 100).integers(0, 256, (10, 12, 3), dtype=np.uint8)
    b = dict(a, C=np.float32([0.0, 0.0, -1000.0]))
    YL, YR, XL, XR, _, _ = a["bound"]
    groups = []
    for Y in range(YL, YR + 1):
        for X in range(XL, XR + 1):
            g = []
            for z in (10.0, 12.0):
                p = on_ray(X, Y, z)
                g.append((p, toward(p, (0, 0, 0))))          # faces pair 0's centre: value 1 there
            groups.append(g)
            groups.append([(on_ray(X, Y, z), TOWARD) for z in (10.0, 8.0, 11.0)])   # faces pair 1 best
    xyz, nrm = _interleave(groups, seed)
    return xyz, nrm, [a, b]


# ---- exhaustive_buckets -----------------------------------------------------------------------------------------------------------
EXH_CZ = -float(2 ** 26)   # CamCenter (0, 0, -2^26): p.z - C.z is rounded to a multiple of 8, so depths 8 j + e (|e| <= 3) tie
LAYOUTS = ("ascending", "descending", "equal")


def _exh_depth(level, passes, alt):
    """Depth on distance level `level` whose column ROUND(z) is even (passes the right mask) or odd."""
    return 8.0 * level + ((2.0 if alt else 0.0) if passes else (3.0 if alt else 1.0))


@functools.lru_cache(maxsize=None)
def _exhaustive_patterns(seed=0):
    W, H = 96, 64
    v = view(W, H, seed, True, C=(0.0, 0.0, EXH_CZ), P1=depth_P1(7), mask1=alternating_mask1(W, H, 7))
    YL, YR, XL, XR, bw, bh = v["bound"]
    pixels = [(XL + t % bw, YL + t // bw) for t in range(bw * bh)]
    cases, groups = [], []
    tie_pairs = {s: list(itertools.combinations(range(s), 2)) for s in (3, 4, 5)}
    n_equal = {3: 0, 4: 0, 5: 0}
    # size 2: both normal relations x all right patterns (depths 20 / 30 + parity)
    for opposite in (False, True):
        for rp in itertools.product((False, True), repeat=2):
            z = [_exh_depth(3 + 2 * k, rp[k], False) for k in range(2)]
            dirs = (True, not opposite)
            cases.append(dict(size=2, opposite=opposite, dirs=dirs, rights=rp, layout="ascending", depths=z))
    for size in (3, 4, 5):
        for dirs in itertools.product((False, True), repeat=size):
            for rp in itertools.product((False, True), repeat=size):
                for layout in LAYOUTS:
                    c = dict(size=size, dirs=dirs, rights=rp, layout=layout)
                    if layout == "equal":
                        a, b = tie_pairs[size][n_equal[size] % len(tie_pairs[size])]
                        n_equal[size] += 1
                        # the tied pair shares a level; the others take distinct levels in an order that changes with the case
                        others = [k for k in range(size) if k not in (a, b)]
                        rot = len(cases) % max(len(others), 1)
                        others = others[rot:] + others[:rot]
                        levels = {a: 6, b: 6}
                        for r, k in enumerate(others):
                            levels[k] = (3, 9, 4)[r] if (len(cases) // 7) % 2 else (9, 3, 8)[r]
                        c["tie"] = (a, b)
                        c["depths"] = [_exh_depth(levels[k], rp[k], k == b) for k in range(size)]
                    else:
                        lv = [2 + 2 * k for k in range(size)]
                        if layout == "descending":
                            lv = lv[::-1]
                        c["depths"] = [_exh_depth(lv[k], rp[k], False) for k in range(size)]
                    cases.append(c)
    assert len(cases) <= len(pixels)
    step = len(pixels) // len(cases)          # spread over the image (and so over the CurrentValue classes)
    for t, c in enumerate(cases):
        X, Y = pixels[t * step] if step > 1 else pixels[t]
        c["pixel"] = (X, Y)
        groups.append([(on_ray(X, Y, c["depths"][k]), TOWARD if c["dirs"][k] else AWAY) for k in range(c["size"])])
    xyz, nrm = _interleave(groups, seed)
    return xyz, nrm, [v], cases


def exhaustive_cases():
    """[dict(pixel, size, dirs, rights, layout, depths[, tie][, opposite])], one pixel each, of exhaustive_buckets("patterns")."""
    return _exhaustive_patterns()[3]


EXTREME_PIXELS = dict(big=(20, 20), alternating=(30, 20), infinite5=(40, 20), infinite3=(41, 20), centre=(10, 10), infinite4=(50, 20))


def exhaustive_buckets(variant="patterns"):
    """patterns: size 2 (both normal relations x 4 right patterns) and sizes 3, 4, 5 (all direction patterns x all right-mask
    patterns x three distance layouts), one pixel per case.  extremes: a 2000-point bucket, a 300-point bucket whose members
    alternate direction along the distance order, buckets with two members at infinite distance, one with two members at the
    camera centre (distance 0)."""
    if variant == "patterns":
        xyz, nrm, views, _ = _exhaustive_patterns()
        return xyz, nrm, views
    assert variant == "extremes"
    W, H = 96, 64
    Cc = on_ray(10, 10, 16.0)
    v = view(W, H, 1, True, C=Cc, P1=depth_P1(7), mask1=alternating_mask1(W, H, 7))
    rng = np.random.default_rng(11)
    E = EXTREME_PIXELS
    groups = []
    rank = rng.permutation(2000)
    groups.append([(on_ray(*E["big"], 17.0 + 0.03 * r), TOWARD if (r // 37) % 2 else AWAY) for r in rank])
    rank = rng.permutation(300)
    groups.append([(on_ray(*E["alternating"], 20.0 + 0.2 * r), TOWARD if r % 2 else AWAY) for r in rank])
    X, Y = E["infinite5"]
    groups.append([(on_ray(X, Y, 30.0), TOWARD), (on_ray(X, Y, 1e20), TOWARD), (on_ray(X, Y, 22.0), TOWARD),
                   (on_ray(X, Y, 2e20), TOWARD), (on_ray(X, Y, 40.0), AWAY)])
    X, Y = E["infinite3"]
    groups.append([(on_ray(X, Y, 2e20), AWAY), (on_ray(X, Y, 24.0), AWAY), (on_ray(X, Y, 1e20), AWAY)])
    X, Y = E["centre"]
    groups.append([(on_ray(X, Y, 20.0), TOWARD), (list(Cc), TOWARD), (on_ray(X, Y, 26.0), TOWARD), (list(Cc), AWAY)])
    X, Y = E["infinite4"]                                # one infinite distance among finite ones
    groups.append([(on_ray(X, Y, 18.0), TOWARD), ([np.float32(X) * np.float32(1e30), np.float32(Y) * np.float32(1e30), np.float32(1e30)], TOWARD),
                   (on_ray(X, Y, 28.0), TOWARD), (on_ray(X, Y, 24.0), TOWARD)])
    xyz, nrm = _interleave(groups, 3)
    return xyz, nrm, [v]


# ---- sorted_array_edges -----------------------------------------------------------------------------------------------------------
# (nv, extra, ((sorted start, size), ...)): nv points get a key, extra points fall in s1 / s2; n = nv + extra
SORTED_VARIANTS = {
    "nv0_n0": (0, 0, ()),
    "nv0_n1": (0, 1, ()),
    "nv1_n1": (1, 0, ()),
    "nv1_n255": (1, 254, ()),
    "nv255_n256": (255, 1, ((62, 3), (252, 3))),
    "nv256_n257": (256, 1, ((63, 5), (253, 3))),
    "nv257_n257": (257, 0, ((62, 5), (254, 3))),
    "nv512_a": (512, 40, ((62, 3), (254, 5), (509, 3))),
    "nv512_b": (512, 0, ((63, 3), (255, 5), (509, 3))),
    "nv512_c": (512, 3, ((61, 5), (256, 5), (507, 5))),
}
SORTED_MASK0_ZERO = (93, 61)     # a bound pixel no bucket uses: left mask 0, the s2 extras land here


def sorted_array_edges(variant):
    """Singleton buckets fill the sorted array; buckets of three and five start at the given sorted positions, so they straddle
    the 64-lane and 256-thread boundaries of the selection kernel's grid or end exactly at nv."""
    nv, extra, starts = SORTED_VARIANTS[variant]
    W, H = 96, 64
    v = view(W, H, 2, False, P1=depth_P1(7), mask1=alternating_mask1(W, H, 7))
    v["mask"][0][SORTED_MASK0_ZERO[1], SORTED_MASK0_ZERO[0]] = 0
    YL, YR, XL, XR, bw, bh = v["bound"]
    sizes, pos, starts = [], 0, dict(starts)
    while pos < nv:
        sizes.append(starts.get(pos, 1))
        pos += sizes[-1]
    assert pos == nv
    depths, dirs = (12.0, 30.0, 21.0, 15.0, 26.0), (TOWARD, AWAY, TOWARD, TOWARD, AWAY)
    groups = []
    for t, s in enumerate(sizes):
        X, Y = XL + (3 * t + 1) % bw, YL + (3 * t + 1) // bw
        groups.append([(on_ray(X, Y, 10.0), TOWARD)] if s == 1 else [(on_ray(X, Y, depths[k]), dirs[(k + t) % 5]) for k in range(s)])
    for e in range(extra):
        groups.append([(on_ray(0, 0, 10.0) if e % 2 == 0 else on_ray(*SORTED_MASK0_ZERO, 10.0), TOWARD)])
    xyz, nrm = _interleave(groups, nv + extra)
    return xyz, nrm, [v]


FAR_CENTRES = [(1e5, 0.0, 0.0), (-1e5, 0.0, 0.0), (0.0, 1e5, 0.0), (0.0, -1e5, 0.0)]


def key_totals(total):
    """Two pairs whose bounds hold 90 x 45 + w x 1 = total keys (4095 / 4096 / 4097: the sentinel and the sorted bit count sit on
    2^12), with points on the first and last key of each pair."""
    w1 = total - 90 * 45
    a = view(96, 64, 4, False, bound=(2, 46, 2, 91, 90, 45), C=FAR_CENTRES[0], P1=depth_P1(7), mask1=alternating_mask1(96, 64, 7))
    b = view(64, 48, 5, False, bound=(5, 5, 3, 3 + w1 - 1, w1, 1), C=FAR_CENTRES[1], P1=depth_P1(7), mask1=alternating_mask1(64, 48, 7))
    groups = []
    for i, vv in enumerate((a, b)):
        YL, YR, XL, XR, _, _ = vv["bound"]
        for (X, Y), zs in (((XL, YL), (10.0,)), ((XR, YR), (12.0, 10.0)), ((XL + 1, YL), (11.0, 12.0)), ((XR - 1, YR), (20.0, 14.0, 17.0))):
            g = []
            for z in zs:
                p = on_ray(X, Y, z)
                g.append((p, toward(p, FAR_CENTRES[i])))
            groups.append(g)
    xyz, nrm = _interleave(groups, total)
    return xyz, nrm, [a, b]


# ---- unequal_pairs ----------------------------------------------------------------------------------------------------------------
UNEQUAL_SIZES = [(40, 30), (96, 64), (64, 48), (48, 40)]
UNEQUAL_BOUNDS = [(2, 27, 2, 37), (5, 50, 7, 80), (2, 45, 3, 61), (4, 37, 2, 40)]     # (YL, YR, XL, XR); pair 0 and 2 touch the 2 px rim
UNEQUAL_VARIANTS = {"full": (), "empty_first": (0,), "empty_middle": (2,), "all_empty": (0, 1, 2, 3)}


def unequal_pairs(variant="full"):
    """Four pairs of different image size and bound.  In every pair: two-point buckets on the bound's four corners whose right
    projections land one pixel outside / on the first and last column (pairs 0, 2) or row (pairs 1, 3) of the right mask, single
    points one pixel outside each side of the bound, and points on left-mask values 0, 1, 254 and 255."""
    views = []
    for i, ((W, H), (YL, YR, XL, XR)) in enumerate(zip(UNEQUAL_SIZES, UNEQUAL_BOUNDS)):
        rng = np.random.default_rng(40 + i)
        m1 = rng.choice(np.uint8([0, 255]), (H, W))
        rows = i % 2 == 1
        if rows:
            m1[0, 3], m1[H - 1, 3] = 255, 255
        else:
            m1[3, 0], m1[3, W - 1] = 255, 255
        bound = (YL, YR, XL, XR, XR - XL + 1, YR - YL + 1)
        v = view(W, H, 30 + i, False, bound=empty_bound(W, H) if i in UNEQUAL_VARIANTS[variant] else bound, C=FAR_CENTRES[i],
                 P1=depth_P1(3, t=-11.0, to_row=rows), mask1=m1)
        for k, val in enumerate((0, 1, 254, 255)):
            v["mask"][0][YL + 3, XL + 3 + k] = val
        views.append(v)
    groups = []
    for i, ((W, H), (YL, YR, XL, XR)) in enumerate(zip(UNEQUAL_SIZES, UNEQUAL_BOUNDS)):
        L = H if i % 2 == 1 else W                    # the right view's moving coordinate is z - 11
        Xm, Ym = (XL + XR) // 2, (YL + YR) // 2
        spots = [((XL, YL), (9.0, 11.0)),                          # -1 (ROUND(-2) = (int)-1.5; miss), 0 (pass)
                 ((XR, YL), (11.0 + L, 10.0 + L)),                 # L (miss), L - 1 (pass)
                 ((XL, YR), (11.0, 9.0)),                          # 0 (pass), -1 (miss)
                 ((XR, YR), (10.0 + L, 11.0 + L, 30.0)),           # L - 1, L, inside: one run of three
                 ((XL - 1, Ym), (20.0,)), ((XR + 1, Ym), (20.0,)), ((Xm, YL - 1), (20.0,)), ((Xm, YR + 1), (20.0,)),
                 ((XL + 3, YL + 3), (20.0,)), ((XL + 4, YL + 3), (20.0, 21.0)), ((XL + 5, YL + 3), (20.0,)), ((XL + 6, YL + 3), (20.0,))]
        for (X, Y), zs in spots:
            g = []
            for z in zs:
                p = on_ray(X, Y, z)
                g.append((p, toward(p, FAR_CENTRES[i])))
            groups.append(g)
    xyz, nrm = _interleave(groups, 9)
    return xyz, nrm, views


# ---- near_ties --------------------------------------------------------------------------------------------------------------------
def near_ties(seed=0, n=4000):
    """Two pairs with centres (-40, 0, -500) and (+40, 0, -500) and 4000 points up to 2e-4 off the mirror plane x = 0, normals in
    that plane: n.(C_i - p) is the same for both pairs and only |C_i - p| tells them apart, in its last bit or not at all.  The
    left views are orthographic ((y, z) -> pixel); pair 0's left mask is 255 and pair 1's is 0 everywhere, so a point that goes
    to pair 0 is emitted (or competes in a bucket) and one that goes to pair 1 counts in s2."""
    W, H = 96, 64
    P0 = np.array([[0, 1.0, 0, 48.0], [0, 0, 1.0, 32.0], [0, 0, 0, 1.0]])
    a = view(W, H, 6, False, C=(-40.0, 0.0, -500.0), P0=P0, P1=P0)
    b = view(W, H, 7, False, C=(40.0, 0.0, -500.0), P0=P0, P1=P0)
    b["mask"][0][:] = 0
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-2e-4, 2e-4, n), rng.uniform(-44.0, 44.0, n), rng.uniform(-28.0, 28.0, n)], 1).astype(np.float32)
    ang = rng.uniform(-0.6, 0.6, n)
    nrm = np.stack([np.zeros(n), np.sin(ang), -np.cos(ang), np.zeros(n)], 1).astype(np.float32)
    return xyz, nrm, [a, b]


# ---- rounding ---------------------------------------------------------------------------------------------------------------------
def _f32_neighbours(q):
    q = np.float32(q)
    return [np.nextafter(q, np.float32(-np.inf)), q, np.nextafter(q, np.float32(np.inf))]


ROUNDING_HALF_PIXEL = (10, 16)     # holds depths 0.49999997 and 1.0: right columns 0 (mask 255) and 1 (mask 0)
ROUNDING_RIGHT_DEPTHS = [0.49999997, 0.5, 1.5, 1.4999999, 1.5000001, -0.5, -0.50000006, -0.49999997, -1.5, -1.4999999, -1.5000001,
                         2.0 ** 31, -(2.0 ** 31), 2147483520.0, -2147483904.0, 2.5, 3.5]


def rounding():
    """One 40x30 pair.  Left view: points (qx, qy, 1), whose quotients are qx and qy exactly: k + 0.5 and its two float neighbours
    for k inside the bound, -0.5 / -1.5 and neighbours, +-2^31 and neighbours, +-inf, NaN, z = 0, z < 0.  Right view (ROUND(z),
    ROUND(z)) with mask 255 on the even diagonal pixels only: two-point buckets (depth d, depth 1.0) on a row of pixels, d from
    ROUNDING_RIGHT_DEPTHS; depth 1.0 always misses (column 1), so the bucket's point d is emitted iff ROUND(d) is even and inside.
    0.49999997f + 0.5 is 0.99999997 in double (column 0) and 1.0f in float (column 1)."""
    W, H = 40, 30
    m1 = np.zeros((H, W), np.uint8)
    for k in range(0, H, 2):
        m1[k, k] = 255
    P1 = np.array([[0, 0, 1.0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])
    v = view(W, H, 8, False, P1=P1, mask1=m1)
    pts, nrm = [], []
    row = 4
    for k in (5.5, 6.5, 20.5):                     # x quotients, one bucket row each
        for q in _f32_neighbours(k):
            pts.append([q, np.float32(row), np.float32(1.0)]); nrm.append(TOWARD)
            row += 1
    for col, k in enumerate((7.5, 8.5, 21.5)):     # y quotients
        for t, q in enumerate(_f32_neighbours(k)):
            pts.append([np.float32(24 + 3 * col + t), q, np.float32(1.0)]); nrm.append(TOWARD)
    for k in (-0.5, -1.5, 2.0 ** 31, -(2.0 ** 31)):
        for q in _f32_neighbours(k):
            pts.append([q, np.float32(5.0), np.float32(1.0)]); nrm.append(TOWARD)
            pts.append([np.float32(5.0), q, np.float32(1.0)]); nrm.append(TOWARD)
    for q in (np.inf, -np.inf, np.nan):
        pts.append([np.float32(q), np.float32(5.0), np.float32(1.0)]); nrm.append(TOWARD)
    pts += [[3.0, 3.0, 0.0], [50.0, 50.0, -10.0], [0.0, 0.0, 0.0]]
    nrm += [TOWARD] * 3
    X0, Y0 = ROUNDING_HALF_PIXEL
    for t, d in enumerate(ROUNDING_RIGHT_DEPTHS):
        for z in (d, 1.0):
            pts.append(on_ray(X0 + t, Y0, z)); nrm.append(TOWARD)
    xyz, nrm = _pack(pts, nrm)
    return xyz, nrm, [v]


FIXTURES = {"minus_one": minus_one, "exhaustive_patterns": lambda: exhaustive_buckets("patterns"),
            "exhaustive_extremes": lambda: exhaustive_buckets("extremes"), "near_ties": near_ties, "rounding": rounding}
FIXTURES.update({"sorted_" + k: functools.partial(sorted_array_edges, k) for k in SORTED_VARIANTS})
FIXTURES.update({"total_%d" % t: functools.partial(key_totals, t) for t in (4095, 4096, 4097)})
FIXTURES.update({"unequal_" + k: functools.partial(unequal_pairs, k) for k in UNEQUAL_VARIANTS})


@functools.lru_cache(maxsize=None)
def get(name):
    """The fixture, built once (callers must not write to it)."""
    return FIXTURES[name]()
