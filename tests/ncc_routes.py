"""The NCC initial match's candidate intervals and the routing of its pixels among its kernels, restated in numpy.

reconstruction_amd/csrc/k_match.hip splits the initial match (LowestLevelInitialMatch / HighLevelInitialMatch,
CStereoMatching.cpp:170-308) among four kernels, and every pixel must reach exactly one of them:
  k_ncc_rowstat   per row: pixels whose interval is longer than ncc_mid ("mid" pixels), the widest interval
  k_ncc_dot4      wide_from = ncc_mid in a row of >= RG_MID_MIN mid pixels, NCC_WIDE otherwise; longer intervals go to a worklist
  k_ncc_wide      the worklist pixels of rows with < RG_MIN of them (one workgroup per pixel, chunks over 8192 workgroups)
  k_rg_rows       the other rows: the sliding sums (k_ncc_slide) when the widest interval is <= ncc_slide_max and the row has
                  >= RG_SLIDE_MIN wide pixels, the int8 row GEMM (k_ncc_rowgemm) otherwise; option wide_rows forces a kernel
This module restates the intervals (mode 0: the other view's margin; mode 1: the carried boundary rule of
oracle/stereo_oracle.c orc_high_level_initial_match, quirk `i + 2 s[i] + offset + 1` included), the routing rule, and
builds the boundary cases of tests/test_gpu_ncc_routes.py.  The GPU tests hold the library's routing witness
(rsm_stage_last_ncc_routes) to `route()` row by row and the disparities to the oracle bit for bit."""
from __future__ import annotations

import math
import os
import re

import numpy as np

NOMATCH = -10000
# the constants of k_match.hip (tests/test_ncc_routes_cpu.py reads them back out of the source)
NCC_TX = 256        # k_ncc_dot4: pixels per workgroup
NCC_WIDE = 160
RG_SLOTS = 512
RG_MIN = 48
RG_SLIDE_MIN = 1024
RG_MID_MIN = 512
RG_PX = 64          # k_ncc_rowgemm: pixels per workgroup
RG_CC = 512         # k_ncc_rowgemm: candidates per staged chunk
SL_COLS = 128       # k_ncc_slide: tile columns (a tile holds SL_COLS - 2R pixels)
SL_DC = 64          # k_ncc_slide: planes per chunk; a workgroup splits its planes 2-way beyond 6 SL_DC, 4-way beyond 12
WIDE_WORKGROUPS = 8192  # k_ncc_wide's grid

ROUTE_NONE, ROUTE_WIDE, ROUTE_GEMM, ROUTE_SLIDE = 0, 1, 2, 3
K_MATCH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reconstruction_amd", "csrc", "k_match.hip")


def default_ncc_mid(r):
    """launch_dot4's ncc_mid when the option is 0: 64 for 11x11 and wider windows, 96 for 7x7 / 9x9, NCC_WIDE (off) below."""
    return 64 if r >= 5 else (96 if r >= 3 else NCC_WIDE)


def options(wide_rows=0, ncc_mid=0, ncc_slide_max=512):
    """The options as rsm_set_option stores them (its clamps)."""
    return dict(wide_rows=wide_rows if 0 <= wide_rows <= 3 else 0,
                ncc_mid=0 if ncc_mid <= 0 else max(8, min(ncc_mid, 160)),
                ncc_slide_max=max(0, min(ncc_slide_max, 1000000)))


def source_constants(path=K_MATCH):
    """The #defines and the ncc_mid default rule as k_match.hip states them."""
    src = open(path).read()
    got = {}
    for name in ("NCC_TX", "NCC_WIDE", "RG_SLOTS", "RG_MIN", "RG_SLIDE_MIN", "RG_MID_MIN", "RG_CC", "SL_COLS", "SL_DC"):
        m = re.search(r"^#define %s (\d+)\b" % name, src, flags=re.M)
        got[name] = int(m.group(1)) if m else None
    m = re.search(r"^#define RG_PX \((\d+) \* (\d+) \* RG_T\)", src, flags=re.M)
    t = re.search(r"^#define RG_T (\d+)\b", src, flags=re.M)
    got["RG_PX"] = int(m.group(1)) * int(m.group(2)) * int(t.group(1)) if m and t else None
    m = re.search(r"if \(a\.ncc_mid <= 0\) a\.ncc_mid = R >= (\d+) \? (\d+) : \(R >= (\d+) \? (\d+) : NCC_WIDE\);", src)
    got["ncc_mid_default"] = tuple(int(g) for g in m.groups()) if m else None   # (5, 64, 3, 96)
    m = re.search(r"hipLaunchKernelGGL\(k_ncc_wide<R>, dim3\((\d+)\)", src)
    got["WIDE_WORKGROUPS"] = int(m.group(1)) if m else None
    m = re.search(r"const int nsplit = pmax > (\d+) \* SL_DC \? 4 : \(pmax > (\d+) \* SL_DC \? 2 : 1\);", src)
    got["slide_split"] = tuple(int(g) for g in m.groups()) if m else None         # (12, 6)
    return got


# ---------------------------------------------------------------- intervals
def intervals(mask_own, own, oth, r, parent=None, offset=2):
    """Per-pixel [L, R] of the candidate scan as the kernels see it, and its width (0: the pixel is not scanned).

    own / oth: margins (YL, YR, XL, XR, ...).  parent None = mode 0 (LowestLevelInitialMatch, .cpp:207: the other margin);
    else mode 1, the carried boundary_L / boundary_R of orc_high_level_initial_match (stereo_oracle.c) on the fp64 parent map.
    Both are clipped to [r, W-1-r] (k_match.hip: windows that would leave the image)."""
    mask_own = np.asarray(mask_own)
    H, W = mask_own.shape
    YL, YR, XL, XR = own[:4]
    XL1, XR1 = oth[2], oth[3]
    L = np.full((H, W), 0x7fffffff, np.int64)
    R = np.full((H, W), -1, np.int64)
    act = np.zeros((H, W), bool)
    if YL <= YR and XL <= XR:
        act[YL:YR + 1, XL:XR + 1] = mask_own[YL:YR + 1, XL:XR + 1] == 255
    if parent is None:
        L[act] = XL1
        R[act] = XR1
    else:
        parent = np.asarray(parent, np.float64)
        for y in range(YL, YR + 1):
            xs = np.nonzero(act[y])[0]
            if xs.size == 0:
                continue
            s = parent[int((y + 1) / 2.0)]
            valid = np.nonzero(s != NOMATCH)[0]
            bl, br = XL1, XR1
            for x in xs:
                t2 = int((x + 1) / 2.0)
                if s[t2] == NOMATCH:
                    j = np.searchsorted(valid, t2 + 1)
                    if j < valid.size and valid[j] <= (XR >> 1):
                        i = int(valid[j])
                        br = min(i + math.trunc(s[i] * 2) + offset + 1, XR1)
                else:
                    c = x + math.trunc(s[t2] * 2 + 0.5)
                    bl = max(c - offset, XL1)
                    br = min(c + offset, XR1)
                L[y, x] = bl
                R[y, x] = br
    L = np.maximum(L, r)
    R = np.minimum(R, W - 1 - r)
    width = np.where(act, np.maximum(R - L + 1, 0), 0)
    return L, R, width


# ---------------------------------------------------------------- routing
def route(width, r, opts):
    """The per-row decision of k_ncc_rowstat / k_ncc_dot4 / k_ncc_wide / k_rg_rows for one direction, in the witness's
    terms: wide, mid, widest, route per row, the worklist length; plus the per-pixel wide map and each row's wide_from."""
    o = options(**opts)
    m = o["ncc_mid"] or default_ncc_mid(r)
    mid = (width > m).sum(1).astype(np.int64)
    widest = width.max(1).astype(np.int64)
    if o["wide_rows"] == 1:           # no k_ncc_rowstat: no mid rows, the counters stay 0
        wide_from = np.full(width.shape[0], NCC_WIDE)
        mid_w, widest_w = np.zeros_like(mid), np.zeros_like(widest)
    else:
        wide_from = np.where(mid >= RG_MID_MIN, m, NCC_WIDE)
        mid_w, widest_w = mid, widest
    wide_px = width > wide_from[:, None]
    wide = wide_px.sum(1).astype(np.int64)
    rt = np.where(wide > 0, ROUTE_WIDE, ROUTE_NONE)
    if o["wide_rows"] != 1:
        listed = wide >= RG_MIN
        if o["wide_rows"] == 2:
            slide = np.zeros_like(listed)
        elif o["wide_rows"] == 3:
            slide = listed
        else:
            slide = listed & (widest <= o["ncc_slide_max"]) & (wide >= RG_SLIDE_MIN)
        rt = np.where(listed, np.where(slide, ROUTE_SLIDE, ROUTE_GEMM), rt)
    return dict(wide=wide, mid=mid_w, widest=widest_w, route=rt, worklist=int(wide.sum()), wide_px=wide_px,
                wide_from=wide_from, ncc_mid=m, mid_all=mid, widest_all=widest, opts=o)


def slide_planes(L, R, wide_px, y, own, r):
    """k_ncc_slide's pre-pass for row y: per workgroup (four tiles of SL_COLS - 2r pixels from the own margin's XL) the
    largest disparity-plane span of a tile's wide pixels, pmax, which picks the 1 / 2 / 4-way plane split."""
    XL, XR = own[2], own[3]
    pxt = SL_COLS - 2 * r
    xs = np.nonzero(wide_px[y])[0]
    if xs.size == 0:
        return []
    tile = (xs - XL) // pxt
    out = []
    for wg in range(int(tile.max()) // 4 + 1):
        pm = 0
        for t in range(4 * wg, 4 * wg + 4):
            sel = xs[tile == t]
            if sel.size:
                pm = max(pm, int((R[y, sel] - sel).max() - (L[y, sel] - sel).min() + 1))
        out.append(pm)
    return out


# ---------------------------------------------------------------- textures and case builders
def texture(kind, W, H, rng):
    if kind == "noise":
        return rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    if kind == "2level":       # two grey levels (tests/test_gpu_ncc_ties.py)
        g = rng.choice(np.array([60, 190], np.uint8), size=(H, W))
        return np.repeat(g[:, :, None], 3, axis=2)
    if kind == "periodic":     # period 7 columns: candidates one period apart tie exactly
        t = rng.integers(0, 256, size=(H, 7, 3)).astype(np.uint8)
        return np.tile(t, (1, (W + 6) // 7, 1))[:, :W]
    raise ValueError(kind)


def _views(kind, W, H, seed, shift):
    rng = np.random.default_rng(seed)
    img0 = texture(kind, W, H, rng)
    img1 = np.roll(img0, shift, axis=1).copy()
    if kind != "noise":       # a few changed pixels so that not every pixel ties
        for _ in range(W * H // 50):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            img1[y, x] = img0[int(rng.integers(0, H)), int(rng.integers(0, W))]
    return img0, img1


def find_margin(mask, r):
    """orc_find_margin (stereo_oracle.c): (YL, YR, XL, XR, width, height) of the 255 pixels at least r from the border."""
    H, W = mask.shape
    sub = mask[r:H - r, r:W - r] == 255
    ys, xs = np.nonzero(sub)
    if ys.size == 0:
        YL, YR, XL, XR = H - 1 - r, r, W - 1 - r, r
    else:
        YL, YR, XL, XR = int(ys.min()) + r, int(ys.max()) + r, int(xs.min()) + r, int(xs.max()) + r
    return (YL, YR, XL, XR, XR - XL + 1, YR - YL + 1)


class Case:
    """One stage call: images, masks, margins, parent (mode 1), the option sets to run it under, and what it is for."""

    def __init__(self, name, r, img_own, img_oth, mask_own, mask_oth, parent=None, offset=2, opt_sets=(), why="", kind="noise",
                 shift=3):
        self.name, self.r, self.offset, self.why, self.kind, self.shift = name, r, offset, why, kind, shift
        self.img_own, self.img_oth, self.mask_own, self.mask_oth = img_own, img_oth, mask_own, mask_oth
        self.parent = parent
        self.H, self.W = mask_own.shape
        self.own, self.oth = find_margin(mask_own, r), find_margin(mask_oth, r)
        self.opt_sets = [options(**o) for o in opt_sets]
        self._iv = None

    @property
    def mode(self):
        return 0 if self.parent is None else 1

    def iv(self):
        if self._iv is None:
            self._iv = intervals(self.mask_own, self.own, self.oth, self.r, self.parent, self.offset)
        return self._iv

    def route(self, opts):
        return route(self.iv()[2], self.r, opts)

    def pairs(self):
        """pixel-candidate pairs the oracle scores (its cost)"""
        return int(self.iv()[2].sum())


def mode0(name, r, W, counts, band, x_start=None, kind="noise", seed=0, shift=3, opt_sets=(), why="", own_cols=None):
    """Lowest-level case: own row i (from row r + 1 on) holds counts[i] active pixels (contiguous from x_start, or the
    columns own_cols[i]); the other mask is the band [band[0], band[1]] in the same rows, so every pixel scans the other
    margin: band clipped to [r, W-1-r] by the margin."""
    H = len(counts) + 2 * r + 2
    m0 = np.zeros((H, W), np.uint8)
    m1 = np.zeros((H, W), np.uint8)
    x0 = 2 * r + 3 if x_start is None else x_start
    for i, n in enumerate(counts):
        y = r + 1 + i
        if own_cols is not None:
            m0[y, own_cols[i]] = 255
        else:
            m0[y, x0:x0 + n] = 255
        m1[y, band[0]:band[1] + 1] = 255
    img0, img1 = _views(kind, W, H, seed, shift)
    return Case(name, r, img0, img1, m0, m1, None, 2, opt_sets, why, kind, shift)


class Mode1Rows:
    """High-level case builder: parent rows of anchors and NOMATCH runs.  A segment (n, w) is an anchor S that sets
    boundary_L, a NOMATCH run of parent columns whose own pixels (n of them) all scan [L_S, L_S + w - 1] (their
    boundary_R comes from the next anchor E: E + trunc(2 s[E]) + offset + 1), and that anchor E; the anchors' own pixels
    scan 2 offset + 1 candidates (or none, when that interval lies outside the other margin).  Own rows 2p-1 and 2p
    share parent row p = p0 + i of design row i (p0: far enough from the border for an r-window)."""

    def __init__(self, W, nrows, r, offset=2, oth_cols=None):
        self.W, self.r, self.offset = W, r, offset
        self.p0 = (r + 3) // 2 + 1
        Hp = self.p0 + nrows + (r + 3) // 2 + 1
        self.H = 2 * Hp
        self.Wp = W // 2 + 2
        self.parent = np.full((Hp, self.Wp), float(NOMATCH))
        self.m0 = np.zeros((self.H, W), np.uint8)
        self.m1 = np.zeros((self.H, W), np.uint8)
        self.oth_cols = oth_cols if oth_cols is not None else (r, W - 1 - r)
        self.XL1, self.XR1 = max(self.oth_cols[0], r), min(self.oth_cols[1], W - 1 - r)

    def _own(self, p, xs):
        for y in (2 * p - 1, 2 * p):
            self.m0[y, xs] = 255
            self.m1[y, self.oth_cols[0]:self.oth_cols[1] + 1] = 255

    def row(self, i, c0, segs, holes=(), lo=None):
        """design row i, first anchor at parent column c0; segs = [(n, w), ...]; holes: own columns masked out;
        lo(n, w, x) -> the L wanted for a run starting at own column x (default: centred on the run where the margin allows)."""
        p = self.p0 + i
        off, c = self.offset, c0
        for n, w in segs:
            S = c
            x_run = 2 * S + 1
            Lw = lo(n, w, x_run) if lo else x_run - w // 2
            Lw = int(min(max(Lw, self.XL1), self.XR1 - w + 1))
            assert Lw >= self.XL1 and Lw + w - 1 <= self.XR1, ("interval does not fit the other margin", n, w)
            q = Lw + off - 2 * S                      # trunc(2 s + 0.5) of S
            self.parent[p, S] = q / 2.0 if q >= 0 else (q - 0.5) / 2.0
            ncol = (n + 1) // 2
            E = S + ncol + 1
            k = Lw + w - E - off - 2                  # trunc(2 s) of E
            self.parent[p, E] = (k + 0.5) / 2.0 if k >= 0 else (k - 0.5) / 2.0
            self._own(p, [2 * S - 1, 2 * S])
            self._own(p, list(range(x_run, x_run + n)))
            self._own(p, [2 * E - 1, 2 * E])
            c = E + 1
        for y in (2 * p - 1, 2 * p):
            self.m0[y, list(holes)] = 0
        return c

    def case(self, name, kind="noise", seed=0, shift=3, opt_sets=(), why=""):
        img0, img1 = _views(kind, self.W, self.H, seed, shift)
        return Case(name, self.r, img0, img1, self.m0, self.m1, self.parent.copy(), self.offset, opt_sets, why, kind, shift)


# ---------------------------------------------------------------- the case set
STD_OPTS = [dict(), dict(wide_rows=1), dict(wide_rows=2), dict(wide_rows=3), dict(ncc_mid=8), dict(ncc_mid=100),
            dict(ncc_mid=160), dict(ncc_slide_max=0), dict(ncc_slide_max=1 << 20)]


def _opts(*extra):
    return STD_OPTS + [dict(e) for e in extra]


def cases():
    cs = []
    # -- interval vs NCC_WIDE in rows below RG_MID_MIN mid pixels; wide count vs RG_MIN (47 / 48)
    for w in (160, 161):
        cs.append(mode0("ncc_wide_w%d_r5" % w, 5, 400, [47, 48, 100, 300, 47, 48], (40, 40 + w - 1), seed=w,
                        opt_sets=_opts(), why="160 / 161 candidates, 47 / 48 wide pixels"))
    # -- mid count vs RG_MID_MIN (511 / 512): a 65-candidate band at R = 5 (ncc_mid 64), 97 at R = 3 (96)
    for r, w in ((5, 65), (3, 97)):
        cs.append(mode0("mid_count_r%d" % r, r, 640, [511, 512, 511, 512], (60, 60 + w - 1), seed=10 + r,
                        opt_sets=_opts(dict(ncc_mid=w - 1), dict(ncc_mid=w)), why="511 / 512 mid pixels"))
    # -- wide count vs RG_SLIDE_MIN (1023 / 1024) and widest vs ncc_slide_max (equal / +1 at 512 and at 200)
    for w in (200, 201, 512, 513):
        cs.append(mode0("slide_w%d_r1" % w, 1, 1100, [1023, 1024, 1024], (30, 30 + w - 1), seed=20 + w,
                        opt_sets=_opts(dict(ncc_slide_max=200), dict(ncc_slide_max=w)), why="1023 / 1024 wide, slide_max"))
    # -- row GEMM candidate chunks: widest 512, 513, 1024, 1025 (RG_CC); XL = 37, not aligned
    for w in (512, 513, 1024, 1025):
        cs.append(mode0("gemm_cc_w%d_r2" % w, 2, 1100, [48, 100, 48], (3, 3 + w - 1), x_start=37, seed=30 + w,
                        opt_sets=_opts(), why="RG_CC chunks"))
    # -- sliding-sum plane split: 48 pixels from XL span 47 columns of one tile (pmax = w + 47), forced to the sliding sums;
    #    1024 pixels from XL fill whole tiles of 128 - 2R pixels (pmax = w + 127 - 2R), taken automatically
    for pm in (384, 385, 768, 769):
        cs.append(mode0("slide_split48_p%d_r2" % pm, 2, 1000, [48, 60], (4, 4 + pm - 47 - 1), x_start=41, seed=40 + pm,
                        opt_sets=_opts(), why="plane split 1 / 2 / 4 ways (wide_rows 3)"))
        w = pm - (SL_COLS - 2 * 1) + 1
        cs.append(mode0("slide_split_p%d_r1" % pm, 1, 1200, [1024, 1030], (5, 5 + w - 1), x_start=43, seed=50 + pm,
                        opt_sets=_opts(), why="plane split, automatic route (ncc_slide_max 1 << 20 for pmax > 512)"))
    # -- more than RG_SLOTS listed rows in one direction: 520 GEMM rows / 520 sliding-sum rows (mid rows at ncc_mid 8)
    cs.append(mode0("slots_gemm_r1", 1, 300, [48] * 520, (10, 170), seed=60, opt_sets=_opts(), why="520 GEMM rows"))
    cs.append(mode0("slots_slide_r1", 1, 1060, [1024] * 520, (10, 18), seed=61,
                    opt_sets=[dict(ncc_mid=8), dict(ncc_mid=8, wide_rows=2), dict(wide_rows=3), dict(ncc_mid=8, ncc_slide_max=9)],
                    why="520 sliding-sum rows"))
    # -- worklist vs k_ncc_wide's 8192 workgroups: 8192 / 8193 entries, some of them in rows k_ncc_wide takes
    for extra in (32, 33):
        cs.append(mode0("worklist_%d" % (8160 + extra), 1, 240, [48] * 170 + [extra], (10, 170), seed=70 + extra,
                        opt_sets=_opts(), why="8192 / 8193 worklist entries"))
    # -- tile edges: a wide pixel first and last in every dot4 (256), GEMM (64) and sliding-sum (128 - 2R) tile, XL odd
    r = 4
    XL = 33
    cols = set()
    for tsz in (NCC_TX, RG_PX, SL_COLS - 2 * r):
        for t in range(0, 1100 // tsz + 1):
            for x in (XL + t * tsz, XL + t * tsz + tsz - 1):
                if x <= XL + 1040:
                    cols.add(x)
    cols = sorted(cols)
    cs.append(mode0("tile_edges_r4", r, 1100, [len(cols)] * 3, (5, 5 + 200), seed=80, own_cols=[cols] * 3,
                    opt_sets=_opts(), why="wide pixels first / last in a tile"))
    cs.append(mode0("tile_edges_full_r4", r, 1100, [1040, 1041], (5, 5 + 300), x_start=XL, seed=81,
                    opt_sets=_opts(), why="whole rows of tiles, XL odd"))
    # -- image-edge clip: bands touching the left / right border, clipped by the margin to exactly 160 / 161 candidates
    for w in (160, 161):
        cs.append(mode0("edge_left_w%d_r3" % w, 3, 420, [60, 48, 47], (0, w + 3 - 1), seed=90 + w,
                        opt_sets=_opts(), why="band from column 0: margin clip lands on %d" % w))
        cs.append(mode0("edge_right_w%d_r6" % w, 6, 420, [60, 48, 47], (420 - w - 6, 419), seed=92 + w,
                        opt_sets=_opts(), why="band to the last column: margin clip lands on %d" % w))
    # -- mode 1, mixed rows at every radius: mid rows with pixels of ncc_mid and ncc_mid + 1 candidates (default, 8, 160),
    #    a mid row of >= 1024 wide pixels (automatic sliding sums), 511 / 512 mid pixels, narrow / masked-out / empty pixels
    for r in range(1, 8):
        m = default_ncc_mid(r) if r >= 3 else 100
        b = Mode1Rows(1400, 5, r)
        blocks = [(520, 161), (16, m), (16, m + 1), (8, 8), (8, 9), (8, 160), (8, 161), (6, 5)]
        b.row(0, 6, blocks, holes=(40, 41, 300))
        b.row(1, 6, [(1030, m + 1), (4, 7)])
        b.row(2, 6, [(511, m + 1), (10, m), (4, 3)])
        b.row(3, 6, [(512, m + 1), (10, m)])
        b.row(4, 6, [(40, 300), (7, 200)])          # 47 wide pixels: k_ncc_wide
        extra = [dict(ncc_mid=m)] if r < 3 else []
        cs.append(b.case("mixed_r%d" % r, seed=100 + r, opt_sets=_opts(*extra, dict(ncc_mid=m, ncc_slide_max=m + 1),
                                                                       dict(ncc_mid=m, ncc_slide_max=m)),
                         why="mode 1 mixed rows, R = %d (ncc_mid %d)" % (r, m)))
    # -- mode 1 textures with ties through every kernel: band, k_ncc_wide, GEMM, sliding sums
    for kind, r, shift in (("periodic", 2, 3), ("2level", 3, -4), ("periodic", 5, -2), ("2level", 5, 5)):
        b = Mode1Rows(1300, 4, r)
        b.row(0, 6, [(30, 200), (10, 5)])           # k_ncc_wide
        b.row(1, 6, [(100, 200), (6, 4)])           # GEMM
        b.row(2, 6, [(1030, 200)])                  # sliding sums
        b.row(3, 6, [(600, 120), (40, 90)])         # mid row (ncc_mid 64 / 96 / option): GEMM
        cs.append(b.case("tex_%s_r%d" % (kind, r), kind=kind, seed=200 + r, shift=shift,
                         opt_sets=_opts(dict(ncc_mid=100)), why="ties from every kernel"))
    return cs


# ---------------------------------------------------------------- coverage of the threshold table
def sides(case, rt, witness=None):
    """The sides of the threshold table (tests/test_gpu_ncc_routes.py) that one (case, options) run reaches: from the
    restatement alone, or with the row-level figures (wide, mid, widest, route, worklist) taken from the library's witness."""
    L, R, width = case.iv()
    if witness is not None:
        rt = dict(rt, wide=witness["wide"].astype(np.int64), route=witness["route"].astype(np.int64), worklist=witness["worklist"])
        if rt["opts"]["wide_rows"] != 1:
            rt["mid_all"], rt["widest_all"] = witness["mid"].astype(np.int64), witness["widest"].astype(np.int64)
    o, r = rt["opts"], case.r
    out = set()
    wr = o["wide_rows"]
    mid_row = (rt["wide_from"] < NCC_WIDE) | ((rt["mid_all"] >= RG_MID_MIN) & (wr != 1))
    non_mid = ~mid_row
    for w in (160, 161):
        if ((width == w) & non_mid[:, None]).any():
            out.add(("NCC_WIDE", w))
    m = rt["ncc_mid"]
    tag = "default" if o["ncc_mid"] == 0 else o["ncc_mid"]
    for w, side in ((m, "=mid"), (m + 1, "=mid+1")):
        if ((width == w) & mid_row[:, None]).any():
            out.add(("ncc_mid", tag, m, side) if tag != "default" else ("ncc_mid", "default", r, side))
    listed = rt["route"] >= ROUTE_GEMM
    if wr != 1:
        for n in (511, 512):
            if (rt["mid_all"] == n).any():
                out.add(("RG_MID_MIN", n))
    if wr == 0:
        for n in (47, 48):
            if (rt["wide"] == n).any():
                out.add(("RG_MIN", n))
        cand = listed & (rt["widest_all"] <= o["ncc_slide_max"])
        for n in (1023, 1024):
            if (cand & (rt["wide"] == n)).any():
                out.add(("RG_SLIDE_MIN", n))
        big = listed & (rt["wide"] >= RG_SLIDE_MIN)
        sm = o["ncc_slide_max"]
        if (big & (rt["widest_all"] == sm)).any():
            out.add(("slide_max", "equal", 512 if sm == 512 else ("0" if sm == 0 else "other")))
        if (big & (rt["widest_all"] == sm + 1)).any():
            out.add(("slide_max", "+1", 512 if sm == 512 else ("0" if sm == 0 else "other")))
        if sm == 0 and big.any():
            out.add(("slide_max", "zero", "0"))
        if (rt["route"] == ROUTE_SLIDE).any():
            out.add(("auto_slide_radius", r))
        if (mid_row & (rt["route"] >= ROUTE_WIDE) & (rt["ncc_mid"] < NCC_WIDE)).any():
            out.add(("mid_route_radius", r))
    gemm = rt["route"] == ROUTE_GEMM
    for w in (512, 513, 1024, 1025):
        if (gemm & (rt["widest_all"] == w)).any():
            out.add(("RG_CC", w))
    for y in np.nonzero(rt["route"] == ROUTE_SLIDE)[0]:
        for pm in slide_planes(L, R, rt["wide_px"], int(y), case.own, r):
            if pm in (384, 385, 768, 769):
                out.add(("slide_split", pm))
    if int(gemm.sum()) > RG_SLOTS:
        out.add(("RG_SLOTS", "gemm"))
    if int((rt["route"] == ROUTE_SLIDE).sum()) > RG_SLOTS:
        out.add(("RG_SLOTS", "slide"))
    if rt["worklist"] in (8192, 8193) and (rt["route"] == ROUTE_WIDE).any():
        out.add(("worklist", rt["worklist"]))
    XL = case.own[2]
    wp = rt["wide_px"]
    ys, xs = np.nonzero(wp)
    k, rel = rt["route"][ys], xs - XL
    for kind, tsz, sel in (("dot4", NCC_TX, np.ones_like(k, bool)), ("gemm", RG_PX, k == ROUTE_GEMM),
                           ("slide", SL_COLS - 2 * r, k == ROUTE_SLIDE)):
        if (sel & (rel % tsz == 0)).any():
            out.add(("tile", kind, "first"))
        if (sel & (rel % tsz == tsz - 1)).any():
            out.add(("tile", kind, "last"))
    if XL % 2 == 1 and wp.any():
        out.add(("tile", "XL unaligned"))
    if case.oth[2] == r and (case.mask_oth[:, :r] == 255).any() or case.oth[3] == case.W - 1 - r and (case.mask_oth[:, -r:] == 255).any():
        ww = case.oth[3] - case.oth[2] + 1
        if ww in (160, 161):
            out.add(("edge_clip", ww))
    return out


def required_sides():
    req = {("NCC_WIDE", 160), ("NCC_WIDE", 161), ("RG_MID_MIN", 511), ("RG_MID_MIN", 512), ("RG_MIN", 47), ("RG_MIN", 48),
           ("RG_SLIDE_MIN", 1023), ("RG_SLIDE_MIN", 1024), ("RG_SLOTS", "gemm"), ("RG_SLOTS", "slide"),
           ("worklist", 8192), ("worklist", 8193), ("edge_clip", 160), ("edge_clip", 161), ("tile", "XL unaligned")}
    for m in (8, 160):
        req |= {("ncc_mid", m, m, "=mid"), ("ncc_mid", m, m, "=mid+1")}
    for r in range(1, 8):
        req |= {("auto_slide_radius", r), ("mid_route_radius", r)}
        if r >= 3:
            req |= {("ncc_mid", "default", r, "=mid"), ("ncc_mid", "default", r, "=mid+1")}
    for v in (512, "other", "0"):
        if v != "0":
            req |= {("slide_max", "equal", v), ("slide_max", "+1", v)}
    req.add(("slide_max", "zero", "0"))
    req |= {("RG_CC", w) for w in (512, 513, 1024, 1025)}
    req |= {("slide_split", p) for p in (384, 385, 768, 769)}
    req |= {("tile", k, s) for k in ("dot4", "gemm", "slide") for s in ("first", "last")}
    return req
