"""Sparse, WIDE depth maps for the cloud filter's wide-window passes (csrc/k_filter.hip: wave_passes, csrc/k_filter_win.hip: k_sor_window_wave / _wg over
windows of 80 ... 2560 pixels; tests/test_gpu_cloud_filter_wide.py).  No GPU here: the maps, the numpy restatement of DisparityToCloud
and of win_clip's bound and window clipping, and what each map claims about itself (tests/test_cloud_lattice_cpu.py checks the
claims, so the GPU tests cannot pass for the wrong reason).

What matters is the lattice's width and height, not the number of points: a margin box of ~2700 x 1400 (or 1400 x 2700) pixels holds
a few thousand points in islands --
  dense patches (40 x 40)       self-sufficient (the list passes or the first wave pass decide them): the hubs the satellites look to;
  hubs                          compact blobs of k + 2 points, the same in small;
  satellites                    3 .. k points whose k + 1 nearest reach into a hub 60, 120, 240, 450, 760 ... 1700 pixels away, along rows,
                                along columns and diagonally: decided by the wave pass whose bound first holds them -- every radius from
                                80 to 2560 (and 5120, the pass that covers the box) decides some;
  satellites beside the sides   their wide windows are clipped to widths such as 2540 and 2494 and at the bottom, so that the window's
                                LARGE candidate indices carry the near neighbours (where the bare multiplication of csrc/win_index.h
                                went wrong);
  lone points, a lone island    fewer than k + 1 points within any window's bound: the whole-cloud search;
and one map of > 65536 points in a thick sheet, which the wave passes must skip whole.
The rig: Q as CStereoMatching::Rectify leaves it, R_final a rotation (identity or not), T_final != 0, focal lengths 3000 and 10000 --
a neighbour d pixels away is within the bound of a window of radius WR only for d < (WR + 1) f / (|D| + WR + 1), |D| >= f."""
import math

import numpy as np

NOMATCH = -10000.0
WIN_PAD = 40                                     # win_bound.h
WAVE_RADII = (80, 160, 320, 640, 1280, 2560, 5120)
KNN_CHUNK, WAVE_LIST, WG_LIST = 1024, 2048, 4096  # knn_select.h: 64 KNN_B candidates a chunk, the wave form's list; k_sor_window_wg's (quarters of 1024)
BASELINE = 100.0


def rig(f, W, H, rotated):
    cx, cy = 0.5 * W - 13.0, 0.5 * H + 7.0
    Q = np.array([[1, 0, 0, -cx], [0, 1, 0, -cy], [0, 0, 0, f], [0, 0, -1.0 / BASELINE, 0]], np.float64)
    if rotated:
        a, b = math.radians(31.0), math.radians(-17.0)
        Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
        R = Ry @ Rx
        T = np.array([350.0, -120.0, 80.0])
    else:
        R = np.eye(3)
        T = np.array([-40.0, 25.0, 10.0])
    return Q, R, T


def blob(u, v, m, wide=3):
    """m pixels in a compact block `wide` columns wide whose first pixel is (u, v)"""
    return [(u + i % wide, v + i // wide) for i in range(m)]


class WideMap:
    """One depth map: .disp (fp64, NOMATCH outside the islands), .mask (all 255: nothing is eroded), .img, .Q / .scale / .R / .T,
    .own (YL, YR, XL, XR, width, height), the islands by name (.islands: name -> list of (x, y) image pixels), what the wave
    passes are expected to do with some named satellites (.expect: name -> radius, None = no window decides it) and the radii at which
    the map claims a wave pass decides some satellite (.covers)."""

    def __init__(self, name, W, H, f, rotated, k, seed, margin=8):
        self.name, self.W, self.H, self.f, self.k = name, W, H, float(f), k
        self.Q, self.R, self.T = rig(f, W, H, rotated)
        self.scale = 1.0
        self.XL, self.XR, self.YL, self.YR = margin, W - 1 - margin, margin + 3, H - 1 - margin
        self.own = (self.YL, self.YR, self.XL, self.XR, self.XR - self.XL + 1, self.YR - self.YL + 1)
        self.gw, self.gh = self.XR - self.XL + 1 + 2 * WIN_PAD, self.YR - self.YL + 1 + 2 * WIN_PAD
        self.disp = np.full((H, W), NOMATCH, np.float64)
        self.mask = np.full((H, W), 255, np.uint8)
        self.img = np.zeros((H, W, 3), np.uint8)
        self.islands, self.expect, self.covers = {}, {}, set()
        self.rng = np.random.default_rng(seed)
        # the disparity: a plane with a gentle slope (1 % across the box) plus noise of 1e-5 relative (a thin sheet: 3-D distances are
        # pixel distances times the lateral spacing B / |d| = 1, nearly)
        self.d0, self.noise = -BASELINE, 1e-5

    def _disp_at(self, x, y):
        slope = 1.0 + 0.01 * (x - self.XL) / self.W - 0.006 * (y - self.YL) / self.H
        return self.d0 * slope * (1.0 + self.noise * self.rng.standard_normal(np.shape(x)))

    def add(self, name, pixels, expect="-"):
        """pixels: (u, v) in BOX coordinates (0, 0 = the margin box's first pixel)"""
        px = [(u + self.XL, v + self.YL) for u, v in pixels]
        for x, y in px:
            assert self.XL <= x <= self.XR and self.YL <= y <= self.YR, (name, x, y)
            assert self.disp[y, x] == NOMATCH, (name, x, y)
            self.disp[y, x] = self._disp_at(np.float64(x), np.float64(y))
        self.islands[name] = px
        if expect != "-":
            self.expect[name] = expect
        return self

    def patch(self, name, u, v, side=40):
        return self.add(name, [(u + i, v + j) for j in range(side) for i in range(side)])

    def hub(self, name, u, v):
        return self.add(name, blob(u, v, self.k + 2))

    def satellite(self, name, u, v, expect="-", m=None):
        return self.add(name, blob(u, v, m if m is not None else max(3, self.k // 3)), expect)

    # ---- the cloud, restated: DisparityToCloud (CStereoMatching.cpp:732-749) in row-major pixel order, cast as InsertPoint casts
    def cloud(self):
        ys, xs = np.nonzero(self.disp[self.YL:self.YR + 1, self.XL:self.XR + 1] != NOMATCH)
        xs, ys = xs + self.XL, ys + self.YL
        d = self.disp[ys, xs]
        q = self.Q.copy()
        q[:, 3] *= self.scale
        iW = 1.0 / (q[3, 3] + q[3, 2] * d)
        F = np.stack([(q[0, 3] + xs) * iW, (ys + q[1, 3]) * iW, q[2, 3] * iW], 1)
        P = F @ self.R.T + self.T
        return P.astype(np.float32), xs, ys

    def index_of(self, xs, ys):
        """{(x, y): cloud index}"""
        return {(int(x), int(y)): i for i, (x, y) in enumerate(zip(xs, ys))}

    # ---- win_clip, restated
    def bound2(self, P32, WR):
        """The largest squared distance a window of radius WR may decide for the float32 points P32 [m, 3] (win_clip's `range`)."""
        P = P32.astype(np.float64)
        dP = P - self.T
        F2 = np.abs(dP @ self.R[:, 2])
        nP = np.sqrt((dP * dP).sum(1))
        iw = F2 / abs(self.Q[2, 3] * self.scale)
        LB = F2 * (WR + 1) / (nP / np.maximum(iw, 1e-300) + (WR + 1))
        coord = np.abs(P).max(1) + nP
        lim = LB * (1.0 - 1e-5) - 4e-7 * coord
        return np.where(lim > 0, lim * lim * (1.0 - 1e-6), 0.0)

    def window(self, x, y, WR):
        """(ncx, ncy, row of the query in the window) of the clipped window of radius WR around image pixel (x, y)"""
        cx, cy = x - self.XL + WIN_PAD, y - self.YL + WIN_PAD
        x0, x1, y0, y1 = max(cx - WR, 0), min(cx + WR, self.gw - 1), max(cy - WR, 0), min(cy + WR, self.gh - 1)
        return x1 - x0 + 1, y1 - y0 + 1, cy - y0

    def first_radius(self, P32, idx, radii=WAVE_RADII, slack=0.02):
        """For the cloud points idx: (tau2 = the squared distance to the (k + 1)-th nearest, the point itself included; the first radius
        of `radii` whose bound holds it, 0 = none; whether that classification has `slack` to spare on both sides)."""
        A = P32[idx].astype(np.float64)
        B = P32.astype(np.float64)
        d2 = sum((A[:, None, a] - B[None, :, a]) ** 2 for a in range(3))
        kth = min(self.k, len(B) - 1)
        tau2 = np.partition(d2, kth, axis=1)[:, kth]
        first = np.zeros(len(idx), np.int64)
        clear = np.ones(len(idx), bool)
        for WR in reversed(radii):
            b2 = self.bound2(P32[idx], WR)
            ok = tau2 < b2
            first = np.where(ok, WR, first)
            clear &= np.abs(tau2 - b2) > slack * b2
        if len(B) <= self.k:   # fewer than k + 1 points in the cloud: no window can hold k + 1
            first[:] = 0
        return tau2, first, clear

    def listed(self, P32, xs, ys, i, WR):
        """The gather of the wave and workgroup forms for cloud point i at radius WR, restated: (K = the candidates of its clipped window
        within the bound -- float32 squared distances below win_clip's `range` --, how many of them each of the workgroup form's four
        waves lists: wave w takes the chunks w, w + 4, ... of KNN_CHUNK row-major candidates)."""
        cx, cy = int(xs[i]) - self.XL + WIN_PAD, int(ys[i]) - self.YL + WIN_PAD
        x0, x1, y0, y1 = max(cx - WR, 0), min(cx + WR, self.gw - 1), max(cy - WR, 0), min(cy + WR, self.gh - 1)
        gx, gy = xs - self.XL + WIN_PAD, ys - self.YL + WIN_PAD
        d = P32[i][None, :] - P32
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == np.float32
        inside = (gx >= x0) & (gx <= x1) & (gy >= y0) & (gy <= y1) & (d2 < np.float32(self.bound2(P32[i:i + 1], WR)[0]))
        c = (gy[inside] - y0) * (x1 - x0 + 1) + (gx[inside] - x0)
        return int(inside.sum()), np.bincount((c // KNN_CHUNK) % 4, minlength=4)


def bare_split_wrong(ncx, ncy):
    """(how many, the first) of the candidates c < ncx * ncy which the multiplication alone (row = umulhi(c, ceil(2^32 / ncx))) splits
    wrongly: uint64 replay; the first is -1 when there is none"""
    c = np.arange(ncx * ncy, dtype=np.uint64)
    inv = np.uint64(0xffffffff // ncx + 1)
    bad = np.nonzero(((c * inv) >> np.uint64(32)) != c // np.uint64(ncx))[0]
    return len(bad), (int(bad[0]) if len(bad) else -1)


# ---- the maps -----------------------------------------------------------------------------------------------------------------
def _satellites_around(m, tag, hu, hv, plan):
    """a dense patch as the hub at box position (hu, hv) and satellites at the offsets of `plan`: (suffix, du, dv)"""
    m.patch(tag + "_hub", hu, hv)
    for suffix, du, dv in plan:
        m.satellite("%s_%s" % (tag, suffix), hu + du, hv + dv)


def wide_f10000(k):
    """2700 x 1400, f = 10000, R_final = I: the radii 80 .. 1280 along rows, columns and diagonals, and a satellite in the lattice's
    first rows that only the pass covering the whole box (5120) reaches a neighbourhood for"""
    m = WideMap("wide_f10000", 2700, 1400, 10000, False, k, 11)
    _satellites_around(m, "r", 2450, 500, [("row60", -62, 0), ("row120", 165, 0), ("col240", 0, -245), ("col450", 0, 495), ("dia240", -175, -175),
                                           ("dia760", -560, 560)])
    m.satellite("corner_tl", 2, 1, 5120)
    m.covers = {80, 160, 320, 640, 1280, 5120}
    return m


def tall_f10000(k):
    """1400 x 2700, f = 10000, rotated rig: the same along columns, and the 2560 pass (neighbours 1400 .. 1700 pixels up the column)"""
    m = WideMap("tall_f10000", 1400, 2700, 10000, True, k, 12)
    _satellites_around(m, "c", 500, 2450, [("col60", 0, -62), ("col120", 0, 168), ("row240", -245, 0), ("row450", 495, 0), ("dia120", 128, -88),
                                           ("dia450", -320, -320), ("col900", 0, -900)])
    m.satellite("far_col1700", 497, 750, 2560)
    m.covers = {80, 160, 320, 640, 1280, 2560}
    return m


def wide_f3000(k):
    """2700 x 1400, f = 3000, rotated rig: satellites beside the sides -- windows clipped to 2540 and 2494 columns, to the lattice's full
    width, and at the bottom"""
    m = WideMap("wide_f3000", 2700, 1400, 3000, True, k, 13)
    # a hub in the last rows and a satellite 760 pixels to its left at box column 1219: at radius 1280 its window is 1219 + 40 + 1280 + 1
    # = 2540 columns wide (clipped at the left side) and clipped at the bottom, the hub in the window's last rows: LARGE candidate indices;
    # the same at box column 1173 (2494 columns) higher up
    m.hub("e_hub1", 1219 + 760, 1340).satellite("edge_2540", 1219, 1352, 1280)
    m.hub("e_hub2", 1173 + 700, 660).satellite("edge_2494", 1173, 665, 1280)
    _satellites_around(m, "s", 2300, 500, [("row60", 102, 0), ("col120", 0, -124), ("dia240", 212, 212), ("col450", 0, 495)])
    m.satellite("far_row1100", 1219 + 760 - 1150, 1300, m=3)   # (2560 for k = 30: clipped at both sides -- the lattice's full width)
    m.satellite("side_left", 1, 700, m=3)                       # (2560 for k = 8, 5120 for k = 30)
    m.covers = {80, 160, 320, 640, 1280, 2560}
    return m


def lone_f3000(k):
    """2700 x 1400, f = 3000, R_final = I: everything but k points sits in the right 600 columns; the k points -- three lone ones in the
    corners and at the left side, and an island -- are more than 1900 pixels from it, beyond the bound of every window"""
    m = WideMap("lone_f3000", 2700, 1400, 3000, False, k, 14)
    m.patch("patch_b", 2600, 1200)
    _satellites_around(m, "s", 2300, 700, [("col60", 0, 103), ("row120", -122, 0), ("col240", 0, -243)])
    m.covers = {80, 160, 320}
    m.add("lone_tl", [(0, 0)], None).add("lone_bl", [(3, 1375)], None).add("lone_ml", [(40, 690)], None)
    m.satellite("lone_island", 150, 300, None, m=k - 3)
    return m


def thick_sheet(k):
    """2700 x 1400, f = 3000: > 65536 points on a 6-pixel grid in a sheet +- 8 % deep -- +- 240 lateral spacings, so that the k + 1 nearest
    of most points lie beyond the bound of the 40-pixel window: more than 65536 queries reach the wave passes, which are skipped whole"""
    m = WideMap("thick_sheet", 2700, 1400, 3000, False, k, 15)
    m.noise = 0.0
    us, vs = np.meshgrid(np.arange(4, 2680, 6), np.arange(4, 1376, 6))
    xs, ys = us.ravel() + m.XL, vs.ravel() + m.YL
    m.disp[ys, xs] = m.d0 * (1.0 + 0.08 * m.rng.uniform(-1.0, 1.0, len(xs)))
    m.islands["sheet"] = list(zip(xs.tolist(), ys.tolist()))
    m.covers = set()
    return m


def dense_f3000(k):
    """660 x 180, f = 3000, R_final = I -- small, but with more candidates within a window's bound than the lists of the wave and workgroup
    forms hold.  `over_a`: 182 pixels beside a 72 x 72 patch, decided at 320 pixels with all 5184 of the patch inside the bound: more than
    the wave form's 2048 and the workgroup form's 4096 -- the histogram narrowing -- and more than 1024 in a quarter -- the workgroup
    form's fallback to one wave's gather.  `fits_b`: 100 pixels beside a 56 x 56 patch, decided at 160 pixels with ~2900 inside the bound:
    the workgroup form's list where the wave form's has overflowed, every quarter within its 1024."""
    m = WideMap("dense_f3000", 660, 180, 3000, False, k, 16)
    m.patch("patch_a", 185, 40, 72).satellite("over_a", 1, 75, 320)
    m.patch("patch_b", 330, 48, 56).satellite("fits_b", 486, 75, 160)
    m.covers = {160, 320}
    return m


MAPS = dict(wide_f10000=wide_f10000, tall_f10000=tall_f10000, wide_f3000=wide_f3000, lone_f3000=lone_f3000)
DENSE_MAPS = dict(dense_f3000=dense_f3000)       # (not wide: apart from test_cloud_lattice_cpu.py's claims about wide boxes)
KS = (8, 30)
