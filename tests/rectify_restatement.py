"""The device part of Rectify (CStereoMatching.cpp:144-158) restated with numpy and scipy, from the geometry and from OpenCV
2.4's published arithmetic -- no GPU, no ctypes, and no line shared with csrc/k_rectify.hip or oracle/rectify_oracle.c.

The kernels (k_rect_map, k_remap<1|3>, k_st_level, k_erode_gray) are compared in tests/test_gpu_rectify.py with the oracle,
whose loops are the kernels' loops character for character: the running sums _x += ir[0], the four guarded taps, the span
rule.  A wrong inverse, a transposed R, a slipped row or a wrong weight that both carry stays unseen there.  Here:
  exact_map     32 u and 32 v of initUndistortRectifyMap from the homography itself, (x, y, w) = (newA R)^-1 (j, i, 1),
                u = fx x / w + u0, in long double (64-bit significand), the inverse refined by two Newton steps
  map_agrees    the fixed-point maps hold rint(32 u), rint(32 v) in every entry; within `delta` of a rounding tie either
                neighbour is accepted (the running sums and the fp64 inverse move 32 u by ~1e-9), and such entries are counted
  fixed_maps    the CV_16SC2 / CV_16UC1 pair that those integers give: >> 5 into int16 (wrapping as the (short) cast does),
                the five low bits of x and of y packed as y * 32 + x
  remap_ref     cv::remap INTER_LINEAR / BORDER_CONSTANT 0 on whole arrays: the source padded by a ring of zeros, the four
                products (32 - fy | fy)(32 - fx | fx) value summed in int64, floor(acc / 1024 + 1 / 2)
  erode_ref     scipy's grey_erosion with getStructuringElement's published ellipse: pair_ends_restatement's, not a third copy
  rectify_ref   the chain of .cpp:154-158
tests/test_rectify_restatement_cpu.py holds these to the oracle and to answers worked out by hand;
tests/test_gpu_rectify_edges.py holds the kernels to them."""
from __future__ import annotations

import numpy as np

from pair_ends_restatement import ellipse_footprint, erode_ref  # noqa: F401  (one copy of the elliptical erosion for all tests)

LD = np.longdouble


# ---------------------------------------------------------------- initUndistortRectifyMap
def exact_map(A, R, newA, W, H):
    """(u32, v32) long double [H, W]: 32 u and 32 v of destination pixel (column j, row i), zero distortion."""
    assert np.finfo(LD).nmant >= 63, "long double carries %d significand bits here: 63 are needed" % np.finfo(LD).nmant
    A, R, newA = (np.asarray(x, np.float64).reshape(3, 3) for x in (A, R, newA))
    M = newA.astype(LD) @ R.astype(LD)
    X = np.linalg.inv(M.astype(np.float64)).astype(LD)
    I = np.eye(3, dtype=LD)
    for _ in range(2):                      # Newton: X <- X + X (I - M X), the residual squares at each step
        X = X + X @ (I - M @ X)
    assert float(np.abs(I - M @ X).max()) < 1e-16          # (the fp64 inverse alone leaves ~1e-13)
    ir = X
    j = np.arange(W, dtype=LD)[None, :]
    i = np.arange(H, dtype=LD)[:, None]
    x = ir[0, 0] * j + ir[0, 1] * i + ir[0, 2]
    y = ir[1, 0] * j + ir[1, 1] * i + ir[1, 2]
    w = ir[2, 0] * j + ir[2, 1] * i + ir[2, 2]
    u = LD(A[0, 0]) * x / w + LD(A[0, 2])
    v = LD(A[1, 1]) * y / w + LD(A[1, 2])
    return LD(32) * u, LD(32) * v


def fixed_maps(u32, v32):
    """(map1 int16 [H, W, 2], map2 uint16 [H, W]) of rint(32 u), rint(32 v): integer part by arithmetic shift, cast to int16
    modulo 2^16; fraction index (iv & 31) * 32 + (iu & 31)."""
    iu = np.rint(u32).astype(np.int64)
    iv = np.rint(v32).astype(np.int64)
    hi_u, hi_v = iu >> 5, iv >> 5
    lo_u, lo_v = iu & 31, iv & 31
    map1 = np.stack([hi_u, hi_v], axis=-1).astype(np.uint16).view(np.int16)   # the low 16 bits, as (short) keeps them
    map2 = (lo_v * 32 + lo_u).astype(np.uint16)
    return map1, map2


_WRAP = 1 << 21   # int16 integer part and five fraction bits: the maps hold iu modulo 2^21


def _rebuild(map1, map2):
    m1 = np.asarray(map1)
    m2 = np.asarray(map2)
    assert m1.dtype == np.int16 and m2.dtype == np.uint16 and m1.shape == m2.shape + (2,)
    m1 = m1.astype(np.int64)
    m2 = m2.astype(np.int64)
    assert int(m2.max(initial=0)) < 1024, "map2 holds bits above the ten of the fraction index"
    return m1[..., 0] * 32 + (m2 & 31), m1[..., 1] * 32 + ((m2 >> 5) & 31)


def near_tie(t32, delta=1e-6):
    """Where 32 u lies within delta of a half-integer."""
    return np.abs(t32 - np.floor(t32) - LD(0.5)) <= LD(delta)


def map_agrees(map1, map2, u32, v32, delta=1e-6):
    """Asserts that every entry of the maps is rint(32 u), rint(32 v) modulo the int16 wrap -- either neighbour where 32 u is
    within delta of a half-integer -- and returns the number of entries excused in that way."""
    excused = np.zeros(np.asarray(map2).shape, bool)
    for name, got, t32 in zip("uv", _rebuild(map1, map2), (u32, v32)):
        assert float(np.abs(t32).max()) < 2.0 ** 31
        want = np.rint(t32).astype(np.int64)
        lo = np.floor(t32).astype(np.int64)
        tie = near_tie(t32, delta)
        ok = (got - want) % _WRAP == 0
        ok |= tie & (((got - lo) % _WRAP == 0) | ((got - lo - 1) % _WRAP == 0))
        if not ok.all():
            bad = np.argwhere(~ok)
            msg = "%d of %d entries of 32 %s are not the rounded exact coordinate" % (len(bad), ok.size, name)
            for (r, c) in bad[:6]:
                msg += "\n   row %d column %d: maps hold %d, 32 %s = %.9f" % (r, c, got[r, c], name, float(t32[r, c]))
            raise AssertionError(msg)
        excused |= tie
    return int(excused.sum())


def map_deviation(map1, map2, u32, v32):
    """The largest |fixed - 32 u| over both coordinates, the int16 wrap undone: 0.5 at most where map_agrees holds."""
    worst = 0.0
    for got, t32 in zip(_rebuild(map1, map2), (u32, v32)):
        d = got.astype(LD) - t32
        d = d - LD(_WRAP) * np.rint(d / LD(_WRAP))
        worst = max(worst, float(np.abs(d).max()))
    return worst


# ---------------------------------------------------------------- remap
def remap_ref(src, map1, map2):
    """cv::remap(src, map1 CV_16SC2, map2 CV_16UC1, INTER_LINEAR, BORDER_CONSTANT 0) on uint8 [Hs, Ws] or [Hs, Ws, 3]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    s = src[..., None] if src.ndim == 2 else src
    Hs, Ws, C = s.shape
    assert C in (1, 3)
    pad = np.zeros((Hs + 2, Ws + 2, C), np.int64)
    pad[1:-1, 1:-1] = s
    m1 = np.asarray(map1).astype(np.int64)
    sx, sy = m1[..., 0], m1[..., 1]
    f = np.asarray(map2).astype(np.int64) & 1023
    fx, fy = f & 31, f >> 5
    acc = np.zeros(f.shape + (C,), np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            px = np.clip(sx + dx + 1, 0, Ws + 1)        # everything outside lands on the ring of zeros
            py = np.clip(sy + dy + 1, 0, Hs + 1)
            acc += (wy * wx)[..., None] * pad[py, px]
    out = (acc + 512) // 1024                            # floor(acc / 1024 + 1 / 2); the weights sum to 1024
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255
    out = out.astype(np.uint8)
    return out[..., 0] if src.ndim == 2 else out


# ---------------------------------------------------------------- the chain
def rectify_ref(raw, maps):
    """Rectify's device part (.cpp:154-158) for both views: raw is a dict with image[2], mask[2] and pyr_levels, maps holds
    (map1, map2) per view.  Returns dict(image, mask): the remapped images, the remapped masks eroded by the ellipse of size
    3 * 2^(PyrmNum - 1)."""
    ksize = 3 * (1 << (int(raw["pyr_levels"]) - 1))
    image, mask = [], []
    for v in range(2):
        m1, m2 = maps[v]
        image.append(remap_ref(raw["image"][v], m1, m2))
        mask.append(erode_ref(remap_ref(raw["mask"][v], m1, m2), ksize))
    return dict(image=image, mask=mask)
