#!/usr/bin/env python
"""Generates tests/golden/ref_probe_golden.npz and tests/golden/ref_stages_golden.npz: seeded inputs + the outputs
the REAL reference produces for them (oracle/_ref/ref_probe = the reference's own CStereoMatching.cpp /
CManageData.cpp objects and its vendored Armadillo 4.200, compiled where they lie; the second fixture's stages
allocate cv::Mat objects on mat_storage.cpp's storage-only stand-in).  Runs only where /root/reference exists; the
.npz files it writes are the committed fixtures, this script is how they were made.

    make -C oracle/ref_probe && python oracle/ref_probe/make_golden.py           # checks ref_probe_golden.npz
    make -C oracle/ref_probe && python oracle/ref_probe/make_golden.py stages    # writes ref_stages_golden.npz
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import blob  # noqa: E402

NOMATCH = -10000


def build_inputs():
    rng = np.random.default_rng(20260929)
    a = {}
    # Armadillo primitives: lengths the path uses (27, 75 = 5x5x3, 363 = 11x11x3, 675) and edge lengths
    for i, n in enumerate([1, 2, 3, 26, 27, 75, 363, 675]):
        v = rng.integers(0, 256, n).astype(np.float64)
        if i == 3:
            v[:] = 17.0  # flat vector -> zero norm after mean removal
        a["arma_vec_%d" % i] = v
        a["arma_vec_b_%d" % i] = rng.normal(0, 50, n)
    meds = [[2, 4, 5, 9], [-9, -5, -4, -2], [3], [7, -1], [1, 2, 3], [5, 5, 6, 6, 7], [-3, -3, 8, 9, 10, 11],
            [-7, 2, -7, 2], [0, -1], [100, -100, 3, 4, 5, 6]]
    for i, m in enumerate(meds):
        a["median_in_%d" % i] = np.array(m, np.int32)
    # WindowToVec
    H, W = 30, 44
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    img[4:9, 10:15] = 93  # a flat 5x5 window (norm 0 -> 1)
    cases = []
    for w in (3, 5, 11):
        for _ in range(8):
            cases.append([int(rng.integers(0, W - w)), int(rng.integers(0, H - w)), w])
    cases.append([10, 4, 5])
    a["w2v_img"] = img
    a["w2v_cases"] = np.array(cases, np.int32)
    # FindMargin
    masks = []
    m = np.zeros((40, 60), np.uint8); m[8:30, 12:50] = 255; m[15, 3] = 255; m[2, 20] = 255; masks.append((m, 2))
    m = np.zeros((40, 60), np.uint8); masks.append((m, 3))                       # empty -> inverted defaults
    m = np.full((33, 47), 255, np.uint8); masks.append((m, 5))                   # full
    m = (rng.random((50, 70)) < 0.03).astype(np.uint8) * 255; m[m == 0] = rng.integers(0, 255, (m == 0).sum()); masks.append((m, 4))
    for i, (mk, r) in enumerate(masks):
        a["fm_mask_%d" % i] = mk
        a["fm_r_%d" % i] = np.array([r], np.int32)
    # OrderConstraint: smooth field + outliers + ties
    for i in range(4):
        Hh, Ww = 20, 90 + 10 * i
        d = (np.round(4 * np.sin(np.arange(Ww) / 9.0))[None, :] + rng.integers(-1, 2, (Hh, Ww))).astype(np.int16)
        out = rng.random((Hh, Ww)) < 0.04 * (i + 1)
        d[out] = rng.integers(-25, 26, out.sum())
        d[rng.random((Hh, Ww)) < 0.2] = NOMATCH
        XL, XR = 3 + i, Ww - 4
        a["oc_disp_%d" % i] = d
        a["oc_margin_%d" % i] = np.array([2, Hh - 3, XL, XR, XR - XL + 1, Hh - 4], np.int32)
    # UniquenessContraint_<short> / <double>
    for i in range(4):
        Hh, Ww = 24, 120
        p = rng.integers(-4, 5, (Hh, Ww)).astype(np.int16)
        q = rng.integers(-4, 5, (Hh, Ww)).astype(np.int16)
        ys, xs = np.nonzero(np.ones_like(p))
        for y, x in list(zip(ys, xs))[::2]:
            t = x + int(p[y, x])
            if 0 <= t < Ww:
                q[y, t] = -p[y, x] + int(rng.integers(-2, 3))
        p[rng.random((Hh, Ww)) < 0.15 + 0.1 * i] = NOMATCH
        q[rng.random((Hh, Ww)) < 0.2] = NOMATCH
        own = [3, Hh - 4, 8, Ww - 9, Ww - 16, Hh - 6]
        oth = [3, Hh - 4, 10, Ww - 12, Ww - 21, Hh - 6]
        if i >= 2:  # double flavour
            pf = np.where(p == NOMATCH, float(NOMATCH), p + rng.normal(0, 0.45, p.shape))
            qf = np.where(q == NOMATCH, float(NOMATCH), q + rng.normal(0, 0.45, q.shape))
            a["uq_p_%d" % i], a["uq_q_%d" % i] = pf, qf
        else:
            a["uq_p_%d" % i], a["uq_q_%d" % i] = p, q
        a["uq_margins_%d" % i] = np.array(own + oth, np.int32)
    build_inputs_round3(a)
    build_inputs_round5(a)
    return a


def build_inputs_round5(a):
    """Round 5: DisparityRefine's data term (.cpp:624-629) -- 3x3x3 windows of whole rows, every (own column, right-window
    left edge) pair: 8-bit noise, a band-limited texture with its shifted + noisy partner (what the bench data look like),
    two- and three-level textures (equal costs reached through different summation orders), flat and saturated regions
    (norm 0 -> 1 on either side, on both)."""
    rng = np.random.default_rng(20261001)
    kinds = ["random", "smooth_shifted", "two_level", "three_level", "flat_regions", "saturated"]
    for i, kind in enumerate(kinds):
        Hh, Ww = 6, 64
        if kind == "random":
            A = rng.integers(0, 256, (Hh, Ww, 3))
            B = rng.integers(0, 256, (Hh, Ww, 3))
        elif kind == "smooth_shifted":
            base = rng.integers(0, 256, (Hh + 4, Ww + 12, 3)).astype(np.float64)
            for _ in range(2):
                base = (base[:, :-4] + 4 * base[:, 1:-3] + 6 * base[:, 2:-2] + 4 * base[:, 3:-1] + base[:, 4:]) / 16
                base = (base[:-2] + 2 * base[1:-1] + base[2:]) / 4
            A = np.round(base[:Hh, :Ww])
            B = np.round(base[:Hh, 3:Ww + 3]) + rng.integers(-2, 3, (Hh, Ww, 3))
        elif kind == "two_level":
            A = rng.choice([0, 255], (Hh, Ww, 1)).repeat(3, 2)
            B = rng.choice([0, 255], (Hh, Ww, 1)).repeat(3, 2)
        elif kind == "three_level":
            A = rng.choice([10, 100, 250], (Hh, Ww, 3))
            B = np.where(rng.random((Hh, Ww, 3)) < 0.7, np.roll(A, 2, axis=1), rng.choice([10, 100, 250], (Hh, Ww, 3)))
        elif kind == "flat_regions":
            A = rng.integers(0, 256, (Hh, Ww, 3)); A[:, 10:20] = 93; A[:, 40:44] = 0
            B = rng.integers(0, 256, (Hh, Ww, 3)); B[:, 15:30] = 93; B[:, 50:] = 255
        else:
            A = rng.integers(200, 300, (Hh, Ww, 3))
            B = rng.integers(-40, 60, (Hh, Ww, 3))
        a["xi_imgA_%d" % i] = np.clip(A, 0, 255).astype(np.uint8)
        a["xi_imgB_%d" % i] = np.clip(B, 0, 255).astype(np.uint8)


def build_inputs_round3(a):
    """Round 3: inputs shaped like what the C2 workload produces (own generator: the entries above keep their bytes)."""
    rng = np.random.default_rng(20260930)
    # FindMargin at the radii of C2 / C5 (5, 7): isolated 255 pixels inside and outside the r-frame, values 254 nearby
    for i, (r, Hh, Ww) in enumerate([(5, 64, 97), (7, 71, 120), (5, 40, 40), (7, 31, 200)], start=4):
        m = rng.integers(0, 255, (Hh, Ww)).astype(np.uint8)          # never 255
        if i != 6:
            m[r + 6:Hh - r - 9, r + 11:Ww - r - 4] = 255
        m[r - 1, Ww // 2] = 255                                      # just outside the scanned frame: ignored
        m[Hh - r, 3] = 255
        m[r, r] = 255 if i == 5 else 254                             # the frame's corner pixel
        m[Hh // 2, Ww - r - 1] = 255                                 # last scanned column
        a["fm_mask_%d" % i] = m
        a["fm_r_%d" % i] = np.array([r], np.int32)
    # OrderConstraint rows with ONE long crossing component (C2's top level: an outlier ties ~2000 pixels together)
    for i, (Ww, nrows) in enumerate([(2100, 3), (2100, 3), (900, 4)], start=4):
        x = np.arange(Ww)
        d = np.round(6 * np.sin(x / 70.0) + 3 * np.sin(x / 13.0))[None, :].repeat(nrows + 4, 0).astype(np.int16)
        d += rng.integers(-1, 2, d.shape).astype(np.int16)
        for y in range(d.shape[0]):
            if i == 4:      # an early pixel thrown far to the right: crosses everything it jumps over
                d[y, 20 + y] = 2000
            elif i == 5:    # a late pixel thrown far to the left, plus a second long jump nested inside the first
                d[y, Ww - 30 - y] = -1990
                d[y, 300] = 1200
            else:           # several medium jumps and equal targets (ties of the crossing count)
                for k in range(6):
                    d[y, 60 + 130 * k] = 400 - 50 * k
                d[y, 500:520] = (519 - np.arange(500, 520)).astype(np.int16) + 500 - 500  # all land on column 519
        d[rng.random(d.shape) < 0.05] = NOMATCH
        XL, XR = 5, Ww - 6
        a["oc_disp_%d" % i] = d
        a["oc_margin_%d" % i] = np.array([2, 2 + nrows - 1, XL, XR, XR - XL + 1, nrows], np.int32)
    # UniquenessContraint<double>: values within 1e-12 of the int(p + 0.5) switch points k - 0.5, both signs, and of
    # the |q + p| < 2 decision
    for i in range(4, 6):
        Hh, Ww = 16, 160
        base = rng.integers(-5, 6, (Hh, Ww)).astype(np.float64)
        eps = rng.choice([0.0, 1e-12, -1e-12, 2.0 ** -40, -2.0 ** -40, 1e-9, -1e-9], (Hh, Ww))
        p = base - 0.5 + eps                                         # p + 0.5 = k + eps
        q = np.zeros((Hh, Ww))
        for y in range(Hh):
            for x in range(Ww):
                q[y, x] = -p[y, max(0, min(Ww - 1, x - int(rng.integers(-5, 6))))] + rng.choice([0.0, 2.0, -2.0, 2.0 - 1e-12, -2.0 + 1e-12, 1.3])
        p[rng.random((Hh, Ww)) < 0.1] = NOMATCH
        q[rng.random((Hh, Ww)) < 0.15] = NOMATCH
        own = [2, Hh - 3, 9, Ww - 10, Ww - 18, Hh - 4]
        oth = [2, Hh - 3, 11, Ww - 13, Ww - 23, Hh - 4]
        a["uq_p_%d" % i], a["uq_q_%d" % i] = p, q
        a["uq_margins_%d" % i] = np.array(own + oth, np.int32)
    # NCC scores of whole rows exactly as the matchers compute them (.cpp:202-211: vecL /= normL;
    # dot(vecL, vecR) / normR): random, two-grey-level, periodic and saturated textures (near and exact ties)
    for i, (r, kind) in enumerate([(2, "random"), (2, "two_level"), (5, "periodic"), (5, "saturated"), (7, "two_level"), (1, "random"),
                                   (1, "two_level_gray"), (2, "three_level"), (1, "three_level")]):
        Hh, Ww = 2 * r + 1 + 3, 72
        if kind == "random":
            A = rng.integers(0, 256, (Hh, Ww, 3))
            B = np.roll(A, 3, axis=1) + rng.integers(-6, 7, A.shape)
        elif kind == "two_level":
            A = rng.choice([40, 200], (Hh, Ww, 1)).repeat(3, 2)
            B = np.roll(A, -2, axis=1)
            B[:, ::7] = 200
        elif kind == "two_level_gray":      # r = 1: few distinct score values, reached through different summation orders
            A = rng.choice([0, 255], (Hh, Ww, 1)).repeat(3, 2)
            B = rng.choice([0, 255], (Hh, Ww, 1)).repeat(3, 2)
        elif kind == "three_level":
            A = rng.choice([10, 100, 250], (Hh, Ww, 3))
            B = np.where(rng.random((Hh, Ww, 3)) < 0.8, np.roll(A, 2, axis=1), rng.choice([10, 100, 250], (Hh, Ww, 3)))
        elif kind == "periodic":
            col = rng.integers(0, 256, (Hh, 8, 3))
            A = np.tile(col, (1, Ww // 8, 1))
            B = np.roll(A, 5, axis=1)
        else:
            A = rng.integers(0, 256, (Hh, Ww, 3))
            A[:, 20:45] = 255
            B = np.roll(A, 4, axis=1)
            B[:, 50:] = 0
        a["ncc_imgA_%d" % i] = np.clip(A, 0, 255).astype(np.uint8)
        a["ncc_imgB_%d" % i] = np.clip(B, 0, 255).astype(np.uint8)
        a["ncc_r_%d" % i] = np.array([r], np.int32)


def _field(rng, H, W, nomatch, outliers=0.04, amp=4.0):
    """A disparity map whose neighbours differ by exactly 0, 1 and 2 (a slow wave + noise in {-1, 0, 1}: DifferOfDisparity's
    threshold, .cpp:3) with a few far outliers, and `nomatch` of its pixels NOMATCH."""
    d = np.round(amp * np.sin(np.arange(W) / 9.0))[None, :] + np.round(np.arange(H) / 7.0)[:, None] + rng.integers(-1, 2, (H, W))
    out = rng.random((H, W)) < outliers
    d[out] = rng.integers(-9, 10, out.sum())
    d = d.astype(np.int16)
    d[rng.random((H, W)) < nomatch] = NOMATCH
    return d


def _mask(rng, H, W, p255):
    """255 with probability p255, every other pixel one of 0..254 (the stages test `!= 255`)."""
    m = rng.integers(0, 255, (H, W)).astype(np.uint8)
    m[rng.random((H, W)) < p255] = 255
    return m


def _mg(YL, YR, XL, XR):
    return [YL, YR, XL, XR, XR - XL + 1, YR - YL + 1]


def build_stage_inputs():
    """The stages that allocate a cv::Mat (SmoothConstraint, MedianFilter, SetBoundary_smooth<short>, Rematch,
    LowestLevelInitialMatch), which run on oracle/ref_probe/mat_storage.cpp's storage.  Own seed, own fixture
    (tests/golden/ref_stages_golden.npz): ref_probe_golden.npz keeps its bytes.  Shapes are the smallest at which the
    kernels' structure can go wrong, see tests/test_oracle_stage_golden.py for what each family must contain."""
    rng = np.random.default_rng(20261018)
    a = {}
    # ---- SmoothConstraint + MedianFilter on the same maps.  Every map is valid outside its margin too (the reference reads
    #      x-1, x+1, y+1 / y-1 there).
    H, W = 37, 151
    sm = [
        (_field(rng, H, W, 0.10), _mg(1, H - 2, 1, W - 2), 0.7),                 # the 1-pixel frame, dense
        (_field(rng, H, W, 0.80), _mg(1, H - 2, 1, W - 2), 0.7),                 # sparse: total == 0 occurs
        (_field(rng, 20, 300, 0.30), _mg(2, 17, 3, 296), 0.8),                   # wider than one 256-thread block, XL = 3
        (_field(rng, H, W, 0.15), _mg(5, 9, 70, 80), 0.9),                       # XL > XR/2: no slip term lands inside
        (_field(rng, H, W, 0.25), _mg(4, 30, 10, 140), 0.8),                     # XL < XR/2: all four slip terms land
        (_field(rng, H, W, 0.50, outliers=0.3, amp=1.5) , _mg(1, H - 2, 1, W - 2), 0.6),   # mixed signs, every window count
        (_field(rng, H, W, 0.35, outliers=0.1, amp=2.0), _mg(3, 33, 2, 147), 1.0),          # all-255 mask
    ]
    sm[5][0][sm[5][0] != NOMATCH] -= 2                                            # centre the values on zero: negative medians
    for i, (d, mg, p255) in enumerate(sm):
        a["sm_disp_%d" % i] = d
        a["sm_mask_%d" % i] = _mask(rng, d.shape[0], d.shape[1], p255)
        a["sm_margin_%d" % i] = np.array(mg, np.int32)
    # ---- SetBoundary_smooth<short>: own-margin (rows, cols) around the kernels' 32-row segments and 64-column chunks, three
    #      fills each; the other view's margin is narrower on both sides, so both clamps act
    i = 0
    for rows, cols in [(2, 70), (3, 64), (31, 63), (32, 128), (33, 129), (97, 321)]:
        YL, XL = 2, 3
        YR, XR = YL + rows - 1, XL + cols - 1
        H, W = YR + 3, XR + 4
        XL1, XR1 = XL + 4, XR - 5
        for fill in range(3):
            if fill == 0:       # 20 % NOMATCH, broken mask
                d, m = _field(rng, H, W, 0.20, outliers=0.1, amp=6.0), _mask(rng, H, W, 0.85)
            elif fill == 1:     # 80 % NOMATCH
                d, m = _field(rng, H, W, 0.80, outliers=0.1, amp=6.0), _mask(rng, H, W, 0.95)
            else:               # one valid pixel under an all-255 mask: a single carry crosses every chunk and segment
                d, m = np.full((H, W), NOMATCH, np.int16), np.full((H, W), 255, np.uint8)
                y0, x0 = [(YL, XL), (YR, XR), ((YL + YR) // 2, (XL + XR) // 2)][i % 3]
                d[y0, x0] = [3, -4, 1][i % 3]
                i += 1
            if fill < 2:
                # .cpp:938-939 assigns: mask 255 at x = XL, not 255 at XL + 1 (nothing arrives from the right), and a right
                # bound that, plus XL, exceeds XR1.  Row YL: nothing arrives at all (the 10000 start value).  Every seventh
                # row from YL + 3 on, in turn: a finite bound, carried down from a disparity that points past XR1, and the
                # start value again (the pixels above and below unmasked).
                d[YL, XL], m[YL, XL], m[YL, XL + 1], m[YL + 1, XL] = NOMATCH, 255, 0, 0
                for j, y in enumerate(range(YL + 3, YR, 7)):
                    if j % 2 == 0:
                        d[y - 1, XL], m[y - 1, XL] = XR1 - XL + 1, 255
                    else:
                        m[y - 1, XL] = 0
                    d[y, XL], m[y, XL], m[y, XL + 1], m[y + 1, XL] = NOMATCH, 255, 0, 0
            k = len([key for key in a if key.startswith("sb_disp_")])
            a["sb_disp_%d" % k], a["sb_mask_%d" % k] = d, m
            a["sb_margins_%d" % k] = np.array(_mg(YL, YR, XL, XR) + _mg(YL, YR, XL1, XR1), np.int32)
    # ---- LowestLevelInitialMatch and Rematch on the same images: radii 1, 2, 5 x four textures, masks with holes in both
    #      views, unequal margins inside the r-frame, three maps for Rematch (2 %, 30 %, 90 % NOMATCH)
    k = 0
    for r in (1, 2, 5):
        for kind in ("random", "two_level", "inverse", "flat_regions"):
            H, W = 2 * r + 1 + 3, 72
            if kind == "random":
                A = rng.integers(0, 256, (H, W, 3))
                B = np.roll(A, 3, axis=1) + rng.integers(-6, 7, A.shape)
            elif kind == "two_level":       # exact ties: the first maximum wins
                A = rng.choice([40, 200], (H, W, 1)).repeat(3, 2)
                B = np.roll(A, -2, axis=1)
                B[:, ::7] = 200
            elif kind == "inverse":         # B = 240 - A: scores at or within a bit of -1, the scan's start value.  The left
                A = rng.choice([40, 200], (H, W, 1)).repeat(3, 2)   # half random, the right half a checkerboard (windows an
                yy, xx = np.mgrid[0:H, 0:W]                          # even shift apart are equal, so EVERY candidate of the
                A[:, W // 2:] = np.where((yy + xx) % 2 == 0, 40, 200)[:, W // 2:, None]   # same parity scores about -1)
                B = 240 - A
            else:                           # flat windows: norm 0 -> 1, score 0
                A = rng.integers(0, 256, (H, W, 3)); A[:, 10:26] = 93; A[:, 50:58] = 0
                B = rng.integers(0, 256, (H, W, 3)); B[:, 18:36] = 93; B[:, 60:] = 255
            A, B = np.clip(A, 0, 255).astype(np.uint8), np.clip(B, 0, 255).astype(np.uint8)
            YL, YR, XL, XR = r, H - 1 - r, r + 1, W - 1 - r - 2
            XL1, XR1 = r + 3, W - 1 - r - 4
            mA, mB = _mask(rng, H, W, 0.85), _mask(rng, H, W, 0.80)
            # a row without a masked candidate inside the other margin (255 only outside it): NOMATCH for the whole row
            mB[YR, XL1:XR1 + 1] = np.minimum(mB[YR, XL1:XR1 + 1], 254)
            mB[YR, :XL1], mB[YR, XR1 + 1:] = 255, 255
            if kind == "inverse":
                # row YL + 1: in the checkerboard half only candidates of one parity are masked, and own pixels of that
                # parity see nothing but scores of about -1
                # (candidate windows wholly inside the checkerboard)
                mB[YL + 1] = np.where((np.arange(W) % 2 == 0) & (np.arange(W) >= W // 2 + r), 255, 0)
                mA[YL + 1, W // 2:] = 255
            # Rematch reads the other view at columns [BL, BR]; both are clamped to the other margin except at x = XL, where
            # .cpp:938-939 leaves BR as it arrived.  Keep the reference inside its rows: wherever the own mask is 255 at XL it
            # is 255 at XL + 1, so BR[XL] <= XR1 arrives from the right ...
            mA[:, XL + 1] = np.where(mA[:, XL] == 255, 255, mA[:, XL + 1])
            mA[YL + 1, XL], mA[YL + 1, XL + 1] = 255, 255
            ds = []
            for nomatch in (0.02, 0.30, 0.90):
                d = _field(rng, H, W, nomatch, outliers=0.08, amp=3.0)
                ds.append(d)
            ds = np.stack(ds)
            # ... except in row YL + 2, built so that the typo fires inside the image: the pixel above carries a disparity that
            # points just past XR1, nothing else arrives, and Rematch scans [XR1, XR1 + 3] -- columns beyond the other margin
            # but inside the r-frame, masked
            y = YL + 2
            mA[y, XL], mA[y, XL + 1], mA[y - 1, XL], mA[y + 1, XL] = 255, 0, 255, 0
            ds[:, y, XL], ds[:, y - 1, XL] = NOMATCH, XR1 + 1 - XL
            mB[y, XR1:XR1 + 4] = 255
            a["mt_imgA_%d" % k], a["mt_imgB_%d" % k] = A, B
            a["mt_maskA_%d" % k], a["mt_maskB_%d" % k] = mA, mB
            a["mt_r_%d" % k] = np.array([r], np.int32)
            a["mt_margins_%d" % k] = np.array(_mg(YL, YR, XL, XR) + _mg(YL, YR, XL1, XR1), np.int32)
            a["mt_disp_%d" % k] = ds
            k += 1
    return a


def run_probe(inputs, probe=None):
    probe = probe or os.path.join(ROOT, "oracle", "_ref", "ref_probe")
    if not os.path.exists(probe):
        subprocess.check_call(["make", "-s", "-C", HERE, "all"])
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.blob"), os.path.join(td, "out.blob")
        blob.write(fi, inputs)
        subprocess.check_call([probe, fi, fo])
        return blob.read(fo)


def main():
    """ref_probe_golden.npz: reruns its inputs through the probe as it is built now and compares every array with the committed
    file, which keeps its bytes: a difference is reported and fails, nothing is rewritten (remove the file by hand to start a
    new one after extending its inputs on purpose)."""
    inputs = build_inputs()
    outputs = run_probe(inputs)
    dst = os.path.join(ROOT, "tests", "golden", "ref_probe_golden.npz")
    new = dict(**{"in__" + k: v for k, v in inputs.items()}, **{"ref__" + k: v for k, v in outputs.items()})
    if os.path.exists(dst):
        old = np.load(dst)
        same = sorted(old.files) == sorted(new)
        for k in sorted(new):
            ok = k in old.files and old[k].dtype == new[k].dtype and old[k].shape == new[k].shape and old[k].tobytes() == new[k].tobytes()
            print("%-28s %-8s %-18s %s" % (k, new[k].dtype, new[k].shape, "identical" if ok else "DIFFERS"))
            same &= ok
        if same:
            print("kept", dst, "-- all", len(new), "arrays identical to the committed fixture")
            return
        sys.exit("the probe no longer reproduces %s: nothing written" % dst)
    np.savez_compressed(dst, **new)
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(outputs), "reference outputs")


def main_stages():
    inputs = build_stage_inputs()
    outputs = run_probe(inputs)
    dst = os.path.join(ROOT, "tests", "golden", "ref_stages_golden.npz")
    np.savez_compressed(dst, **{"in__" + k: v for k, v in inputs.items()}, **{"ref__" + k: v for k, v in outputs.items()})
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(outputs), "reference outputs")


if __name__ == "__main__":
    if sys.argv[1:] == ["stages"]:
        main_stages()
    else:
        main()
