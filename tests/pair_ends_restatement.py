"""The two ends of a pair restated with numpy and scipy: pyrDown, the elliptical erosion, the NCC window-sum tables and
DisparityToCloud -- and the constructed inputs the CPU and GPU tests of them share.

reconstruction_amd/csrc/k_pyramid.hip and k_cloud.hip are compared in the parity tests with oracle/stereo_oracle.c, whose
pyrDown and erosion are restatements themselves and share reflect101, the weights, the rounding and the span rule with the
kernels.  The references here share none of that code:
  pyr_down_ref    scipy.ndimage.correlate1d with [1 4 6 4 1] and mode='mirror' (BORDER_REFLECT_101) along both axes in int64,
                  every second sample, (v + 128) >> 8
  erode_ref       scipy.ndimage.grey_erosion with the footprint of getStructuringElement(MORPH_ELLIPSE) from its published
                  formula; pixels outside the image are 255, i.e. ignored, as cv::erode's default border is
  box_sums_ref    summed-area tables of the per-pixel byte sums and sums of squares
  cloud_ref       DisparityToCloud (CStereoMatching.cpp:682-761) in elementwise fp64 on whole arrays, same expression tree
tests/test_pair_ends_cpu.py holds them to the oracle and to answers written by hand, tests/test_gpu_pair_ends.py holds the
kernels to them."""
from __future__ import annotations

import math

import numpy as np
from scipy import ndimage

from ncc_routes import find_margin  # noqa: F401  (the FindMargin restatement: one copy for all tests)

NOMATCH = -10000


# ---------------------------------------------------------------- pyrDown
def pyr_down_ref(a):
    """cv::pyrDown on uint8 [H, W] or [H, W, C]: dst = ((H + 1) / 2, (W + 1) / 2)."""
    a = np.asarray(a)
    assert a.dtype == np.uint8
    v = a.astype(np.int64)
    k = np.array([1, 4, 6, 4, 1], np.int64)
    v = ndimage.correlate1d(v, k, axis=0, mode="mirror")
    v = ndimage.correlate1d(v, k, axis=1, mode="mirror")
    v = v[::2, ::2]
    return ((v + 128) >> 8).astype(np.uint8)


# ---------------------------------------------------------------- erosion by an ellipse
def ellipse_footprint(k):
    """getStructuringElement(MORPH_ELLIPSE, (k, k)): row i holds ones in [c - dx, c + dx], r = c = k / 2,
    dx = round_half_even(c sqrt((r^2 - dy^2) / r^2)), dy = i - r; rows with |dy| > r are empty; k = 1 is a single one."""
    k = int(k)
    fp = np.zeros((k, k), bool)
    r = c = k // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    for i in range(k):
        dy = i - r
        if abs(dy) > r:
            continue
        dx = int(np.rint(c * math.sqrt((r * r - dy * dy) * inv_r2)))
        fp[i, max(c - dx, 0):min(c + dx + 1, k)] = True
    return fp


def erode_ref(mask, k):
    """cv::erode(mask, ellipse(k)) with the default anchor (k / 2, k / 2) and border (ignored pixels)."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2
    return ndimage.grey_erosion(mask, footprint=ellipse_footprint(k), mode="constant", cval=255)


# ---------------------------------------------------------------- window sums
def box_sums_ref(img_bgr, r):
    """(S1, S2) int64 [H, W]: sum and sum of squares of the (2r+1) x (2r+1) x 3 bytes centred on the pixel; 0 where the
    window does not fit into the image."""
    img = np.asarray(img_bgr)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    H, W = img.shape[:2]
    v = img.astype(np.int64)
    w = 2 * r + 1
    out = []
    for p in (v.sum(axis=2), (v * v).sum(axis=2)):
        ii = np.zeros((H + 1, W + 1), np.int64)
        ii[1:, 1:] = p.cumsum(axis=0).cumsum(axis=1)
        S = np.zeros((H, W), np.int64)
        if H >= w and W >= w:
            S[r:H - r, r:W - r] = ii[w:, w:] - ii[:-w, w:] - ii[w:, :-w] + ii[:-w, :-w]
        assert S.min() >= 0 and S.max() < 2 ** 31
        out.append(S)
    return out[0], out[1]


# ---------------------------------------------------------------- DisparityToCloud
def cloud_selection(d, mask, own):
    """The pixels DisparityToCloud emits: inside the margin, d != NOMATCH, eroded mask == 255 (boolean [H, W])."""
    d = np.asarray(d, np.float64)
    H, W = d.shape
    YL, YR, XL, XR = own[:4]
    ksize = int(math.ceil(0.02 * H))
    sel = np.zeros((H, W), bool)
    if YL <= YR and XL <= XR:
        sel[YL:YR + 1, XL:XR + 1] = True
    sel &= d != NOMATCH
    sel &= erode_ref(np.asarray(mask), ksize) == 255
    return sel


def cloud_ref(d, mask, img, Q, scale, R, T, own):
    """(xyz float64 [n, 3], bgr uint8 [n, 3]) in row-major pixel order."""
    d = np.asarray(d, np.float64)
    q = np.array(Q, np.float64).reshape(4, 4).copy()
    q[:, 3] *= scale
    R = np.asarray(R, np.float64).reshape(3, 3)
    T = np.asarray(T, np.float64).reshape(3)
    ys, xs = np.nonzero(cloud_selection(d, mask, own))   # row-major
    dv = d[ys, xs]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iW = 1.0 / (q[3, 3] + q[3, 2] * dv)
        F0 = (q[0, 3] + xs.astype(np.float64)) * iW
        F1 = (ys.astype(np.float64) + q[1, 3]) * iW
        F2 = q[2, 3] * iW
        xyz = np.stack([(R[i, 0] * F0 + R[i, 1] * F1 + R[i, 2] * F2) + T[i] for i in range(3)], axis=1)
    return xyz.reshape(-1, 3), np.asarray(img)[ys, xs].reshape(-1, 3).copy()


# ---------------------------------------------------------------- shared inputs
PYR_SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 7), (7, 1), (2, 9), (3, 4), (4, 5), (5, 5), (9, 2), (17, 33),
             (64, 511), (33, 513), (31, 1025)]   # (H, W); the last three cross the kernel's 256-wide destination blocks
PYR_KINDS = ("random", "binary", "white")


def pyr_image(H, W, C, kind):
    rng = np.random.default_rng(1000003 * H + 1009 * W + 7 * C + len(kind))
    shape = (H, W) if C == 1 else (H, W, C)
    if kind == "random":
        return rng.integers(0, 256, size=shape).astype(np.uint8)
    if kind == "binary":
        return rng.choice(np.array([0, 255], np.uint8), size=shape)
    return np.full(shape, 255, np.uint8)


def pyr_cases():
    """(H, W, C, kind) for every size, 1 and 3 channels, the three kinds of image."""
    return [(H, W, C, kind) for (H, W) in PYR_SIZES for C in (1, 3) for kind in PYR_KINDS]


ERODE_KS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 17, 24, 34, 40, 61]
ERODE_SIZES = [(1, 1), (7, 5), (33, 64), (70, 45), (130, 97)]   # (H, W)


def erode_mask(H, W, seed):
    """255 with ~3 % non-255 pixels of any value and a few solid patches: holes smaller and larger than the elements."""
    rng = np.random.default_rng(seed)
    m = np.full((H, W), 255, np.uint8)
    bad = rng.random((H, W)) < 0.03
    m[bad] = rng.integers(0, 255, size=int(bad.sum()))
    for _ in range(3):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        m[y:y + int(rng.integers(1, 6)), x:x + int(rng.integers(1, 6))] = int(rng.integers(0, 255))
    return m


BOX_RADII = [1, 2, 3, 4, 5, 6, 7, 8, 12, 15]   # every k_box_h<R> template and k_box_h_any


def box_sizes(r):
    """(H, W): one defined pixel; all zero both ways; defined rows that start mid-chunk of the vertical pass and span two
    chunks; widths around the 1024 columns of a horizontal block with W mod 4 = 3, 1, 2 (and 2r + 2 / 40 / 2r + 1 else)."""
    return [(2 * r + 1, 2 * r + 1), (2 * r, 40), (40, 2 * r), (2 * r + 18, 2 * r + 2), (33, 1023), (18, 1025), (2 * r + 35, 1030)]


def box_image(H, W, kind, seed=0):
    if kind == "white":
        return np.full((H, W, 3), 255, np.uint8)
    return np.random.default_rng(7919 * H + 31 * W + seed).integers(0, 256, size=(H, W, 3)).astype(np.uint8)


# (H, W, YL, YR, XL, XR): row counts 294 / 1696 (k_row_scan's 256-row chunks) and 257, margin widths 521 / 257 (the
# 256-column ballot chunks), ksize = ceil(0.02 H) = 6 / 2 / 34 / 6 / 1 (34 > the quick-accept block of 32), a one-row margin
CLOUD_GEOMS = [(300, 40, 3, 296, 2, 37), (60, 600, 5, 50, 10, 530), (1700, 70, 2, 1697, 2, 67), (257, 258, 0, 256, 1, 257),
               (50, 50, 10, 10, 5, 44)]
CLOUD_SHARES = [0.0, 0.03, 0.5, 1.0]
CLOUD_MASKS = ("patches", "white", "none")


def cloud_calibration(W, H, seed):
    """A Q of the pipeline's shape (column 3 gets scaled), a rotation about two axes and a translation; no entry is 0 or 1
    where the reference multiplies, so that every product and sum of the expression tree rounds."""
    f = 1.2371 * W
    Q = np.array([[1, 0, 0, -(W / 2.0 + 0.37)], [0, 1, 0, -(H / 2.0 - 0.21)], [0, 0, 0, f], [0, 0, -1.0 / 97.3, 0.013]], np.float64)
    a, b = 0.3 + 0.1 * seed, -0.7 + 0.05 * seed
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    return Q, Ry @ Rx, np.array([311.7, -42.3, 97.1]) * (1 + seed), 0.83


def cloud_input(geom, share, mask_kind, seed=0):
    """dict(d, mask, img, Q, scale, R, T, own) for one constructed DisparityToCloud call.

    d: fp64, `share` of the pixels valid (uniform in [-40, 40), a tenth of them rounded to integers), NOMATCH elsewhere.
    With share > 0 one valid pixel of the margin carries d == 0; in the geometries of even index q33 is 0, as in the
    pipeline's own Q, and that pixel is 1 / 0: the reference divides all the same (.cpp:745) and emits a non-finite point.
    In the others q33 != 0 and the denominator's sum rounds.
    mask "patches": 255 with eight small random non-255 patches, a 254 first column and non-255 pixels at (0, 0), (31, 31),
    (32, 32), (H-1, W-1), the corners of the quick-accept blocks; "white": all 255; "none": no 255 at all."""
    H, W, YL, YR, XL, XR = geom
    rng = np.random.default_rng(100 * (CLOUD_GEOMS.index(geom) + 1) + 10 * CLOUD_SHARES.index(share) + CLOUD_MASKS.index(mask_kind) + 1000 * seed)
    Q, R, T, scale = cloud_calibration(W, H, CLOUD_GEOMS.index(geom))
    d = np.full((H, W), float(NOMATCH))
    v = rng.random((H, W)) < share
    d[v] = rng.uniform(-40, 40, size=int(v.sum()))
    ints = v & (rng.random((H, W)) < 0.1)
    d[ints] = np.round(d[ints])
    if mask_kind == "white":
        m = np.full((H, W), 255, np.uint8)
    elif mask_kind == "none":
        m = rng.integers(0, 255, size=(H, W)).astype(np.uint8)
    else:
        m = np.full((H, W), 255, np.uint8)
        for _ in range(8):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            m[y:y + int(rng.integers(1, 5)), x:x + int(rng.integers(1, 5))] = int(rng.integers(0, 255))
        m[:, 0] = 254
        for (y, x) in ((0, 0), (31, 31), (32, 32), (H - 1, W - 1)):
            if y < H and x < W:
                m[y, x] = int(rng.integers(0, 255))
    if CLOUD_GEOMS.index(geom) % 2 == 0:
        Q[3, 3] = 0.0
    if share > 0:                                # among the pixels that are emitted, so that the point is in the cloud
        ys, xs = np.nonzero(cloud_selection(d, m, (YL, YR, XL, XR)))
        if ys.size:
            i = int(rng.integers(0, ys.size))
            d[ys[i], xs[i]] = 0.0
    img = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    return dict(d=d, mask=m, img=img, Q=Q, scale=scale, R=R, T=T, own=(YL, YR, XL, XR, XR - XL + 1, YR - YL + 1))


def cloud_cases():
    """(geom, share, mask_kind): every geometry and share with the patched mask; the all-255 and the no-255 mask once per
    geometry (share 0.5)."""
    out = [(g, s, "patches") for g in CLOUD_GEOMS for s in CLOUD_SHARES]
    out += [(g, 0.5, k) for g in CLOUD_GEOMS for k in ("white", "none")]
    return out


_cloud_refs = {}


def cloud_reference(case):
    """(input dict, (xyz, bgr) of cloud_ref) of one case, computed once per process and not to be written to."""
    if case not in _cloud_refs:
        inp = cloud_input(*case)
        _cloud_refs[case] = (inp, cloud_ref(**inp))
    return _cloud_refs[case]


def cloud_case_id(c):
    g, s, k = c
    return "%dx%d_share%g_%s" % (g[0], g[1], s, k)


def same_values(a, b):
    """fp64 arrays equal bit for bit wherever either holds a number (infinities and signed zeros included), and NaN in the
    same places: which NaN an invalid operation returns (sign, payload) is the processor's choice, not IEEE 754's."""
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))
