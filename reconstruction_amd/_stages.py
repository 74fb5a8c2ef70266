"""The per-stage entry points the parity tests drive (csrc/rsm_stages.hip): one direction, host buffers in and out."""
import ctypes as C

import numpy as np

from . import _lib
from ._context import ContextBase, _bd, _p, _u8
from ._lib import Boundary


class StagesPart(ContextBase):
    def rect_map(self, A, R, newA, W, H):
        A, R, newA = (np.ascontiguousarray(x, np.float64) for x in (A, R, newA))
        m1 = np.zeros((H, W, 2), np.int16); m2 = np.zeros((H, W), np.uint16)
        self._chk(self._lib.rsm_stage_rect_map(self._h, _p(A), _p(R), _p(newA), W, H, _p(m1), _p(m2)))
        return m1, m2

    def remap_linear(self, src, map1, map2):
        src = _u8(src); Hs, Ws = src.shape[:2]; ch = 1 if src.ndim == 2 else src.shape[2]
        H, W = map2.shape
        m1 = np.ascontiguousarray(map1, np.int16); m2 = np.ascontiguousarray(map2, np.uint16)
        dst = np.zeros((H, W) + (() if src.ndim == 2 else (ch,)), np.uint8)
        self._chk(self._lib.rsm_stage_remap(self._h, _p(src), Ws, Hs, ch, _p(m1), _p(m2), W, H, _p(dst)))
        return dst

    def _erode(self, fn, mask, ksize):
        mask = _u8(mask); H, W = mask.shape
        dst = np.zeros_like(mask)
        self._chk(fn(self._h, _p(mask), W, H, ksize, _p(dst)))
        return dst

    def erode_ellipse_gray(self, mask, ksize):
        return self._erode(self._lib.rsm_stage_erode_gray, mask, ksize)

    def bench_ncc(self, W, H, r, cands, iters=5) -> float:
        ms = C.c_double()
        self._chk(self._lib.rsm_bench_ncc(self._h, W, H, r, cands, iters, C.byref(ms)))
        return ms.value

    def find_margin(self, mask, r):
        mask = _u8(mask); H, W = mask.shape
        m = Boundary()
        self._chk(self._lib.rsm_stage_find_margin(self._h, _p(mask), W, H, r, C.byref(m)))
        return m

    def pyr_down(self, src):
        src = _u8(src); H, W = src.shape[:2]
        ch = 1 if src.ndim == 2 else src.shape[2]
        dst = np.zeros(((H + 1) // 2, (W + 1) // 2) + (() if src.ndim == 2 else (ch,)), np.uint8)
        self._chk(self._lib.rsm_stage_pyr_down(self._h, _p(src), W, H, ch, _p(dst)))
        return dst

    def erode_ellipse_is255(self, mask, ksize):
        return self._erode(self._lib.rsm_stage_erode_ellipse, mask, ksize)

    def box_sums(self, img, r):
        """The NCC window-sum tables (S1, S2) of a BGR image, int32 [H, W] (include/rsm.h rsm_stage_box_sums)."""
        img = _u8(img); H, W = img.shape[:2]
        assert img.shape == (H, W, 3)
        S1 = np.zeros((H, W), np.int32); S2 = np.zeros((H, W), np.int32)
        self._chk(self._lib.rsm_stage_box_sums(self._h, _p(img), W, H, int(r), _p(S1), _p(S2)))
        return S1, S2

    def initial_match(self, img_own, img_oth, mask_own, mask_oth, r, offset, own, oth, parent=None):
        img_own, img_oth, mask_own, mask_oth = map(_u8, (img_own, img_oth, mask_own, mask_oth))
        H, W = mask_own.shape
        d = np.zeros((H, W), np.int16)
        if parent is None:
            pp, Wp, Hp = None, 0, 0
        else:
            parent = np.ascontiguousarray(parent, np.float64)
            Hp, Wp = parent.shape
            pp = _p(parent)
        self._chk(self._lib.rsm_stage_initial_match(self._h, _p(img_own), _p(img_oth), _p(mask_own), _p(mask_oth), W, H, r, offset, C.byref(_bd(own)),
                                                    C.byref(_bd(oth)), pp, Wp, Hp, _p(d)))
        return d

    def last_ncc_routes(self, H):
        """What the last initial_match decided per row (include/rsm.h rsm_stage_last_ncc_routes): dict of int32 arrays
        wide / mid / widest / route (0 none, 1 workgroup per pixel, 2 int8 row GEMM, 3 sliding sums) and the ints
        worklist, ties."""
        out = {k: np.zeros(H, np.int32) for k in ("wide", "mid", "widest", "route")}
        wl, ti = C.c_int64(), C.c_int64()
        self._chk(self._lib.rsm_stage_last_ncc_routes(self._h, int(H), _p(out["wide"]), _p(out["mid"]), _p(out["widest"]), _p(out["route"]), C.byref(wl),
                                                      C.byref(ti)))
        out["worklist"], out["ties"] = int(wl.value), int(ti.value)
        return out

    def _constraint(self, fn, disp, own):
        d = np.array(disp, dtype=np.int16, order="C"); H, W = d.shape
        self._chk(fn(self._h, _p(d), W, H, C.byref(_bd(own))))
        return d

    def smooth_constraint(self, disp, own):
        return self._constraint(self._lib.rsm_stage_smooth, disp, own)

    def order_constraint(self, disp, own):
        return self._constraint(self._lib.rsm_stage_order, disp, own)

    def uniqueness_pass(self, p, q, own, oth):
        if np.asarray(p).dtype == np.float64:
            p = np.array(p, dtype=np.float64, order="C"); q = np.ascontiguousarray(q, np.float64)
            fn = self._lib.rsm_stage_uniqueness_pass_f64
        else:
            p = np.array(p, dtype=np.int16, order="C"); q = np.ascontiguousarray(q, np.int16)
            fn = self._lib.rsm_stage_uniqueness_pass_s16
        H, W = p.shape
        self._chk(fn(self._h, _p(p), _p(q), W, H, C.byref(_bd(own)), C.byref(_bd(oth))))
        return p

    def uniqueness(self, d0, d1, m0, m1):
        """UniquenessContraint<T> (.cpp:450-461): three passes."""
        d0 = self.uniqueness_pass(d0, d1, m0, m1)
        d1 = self.uniqueness_pass(d1, d0, m1, m0)
        d0 = self.uniqueness_pass(d0, d1, m0, m1)
        return d0, d1

    def set_boundary_smooth(self, disp, mask_own, own, oth):
        d = np.ascontiguousarray(disp, np.int16); mask_own = _u8(mask_own); H, W = d.shape
        BL = np.zeros((H, W), np.int16); BR = np.zeros((H, W), np.int16)
        st = self._lib.rsm_stage_set_boundary(self._h, _p(d), _p(mask_own), W, H, C.byref(_bd(own)), C.byref(_bd(oth)), _p(BL), _p(BR))
        if st not in (0, _lib.RSM_E_DEGENERATE_MARGIN):
            self._chk(st)
        return st, BL, BR

    def rematch(self, img_own, img_oth, mask_own, mask_oth, r, own, oth, disp):
        img_own, img_oth, mask_own, mask_oth = map(_u8, (img_own, img_oth, mask_own, mask_oth))
        d = np.array(disp, dtype=np.int16, order="C"); H, W = d.shape
        st = self._lib.rsm_stage_rematch(self._h, _p(img_own), _p(img_oth), _p(mask_own), _p(mask_oth), W, H, r, C.byref(_bd(own)), C.byref(_bd(oth)), _p(d))
        if st not in (0, _lib.RSM_E_DEGENERATE_MARGIN):
            self._chk(st)
        return st, d

    def median_filter(self, disp, mask_own, own):
        d = np.array(disp, dtype=np.int16, order="C"); mask_own = _u8(mask_own); H, W = d.shape
        self._chk(self._lib.rsm_stage_median(self._h, _p(d), _p(mask_own), W, H, C.byref(_bd(own))))
        return d

    def disparity_refine(self, disp, img_own, img_oth, iterations, ws, own):
        d = np.ascontiguousarray(disp, np.int16); img_own = _u8(img_own); img_oth = _u8(img_oth)
        H, W = d.shape
        out = np.zeros((H, W), np.float64)
        self._chk(self._lib.rsm_stage_refine(self._h, _p(d), _p(img_own), _p(img_oth), W, H, iterations, ws, C.byref(_bd(own)), _p(out)))
        return out

    def exp_neg(self, t, small_form: bool = False):
        """The specified exp(-t) of DisparityRefine's smoothness weights, evaluated on the device (small_form: through the
        time-skewed kernel's common-path form for arguments below 512)."""
        t = np.ascontiguousarray(t, np.float64).ravel()
        out = np.zeros(t.shape, np.float64)
        fn = self._lib.rsm_stage_exp_neg_small if small_form else self._lib.rsm_stage_exp_neg
        self._chk(fn(self._h, _p(t), t.size, _p(out)))
        return out

    def refine_xi(self, img_own, img_oth, form: int = 0):
        """DisparityRefine's matching costs xi (CStereoMatching.cpp:624-629) as the device computes them: array [3, H-2, W-2, W-2],
        [c, y-1, x-1, col] = xi(x, y, col + c); form 0 / 1 / 2 = the first sweep's / lane-per-miss / four-lanes-per-miss routine."""
        img_own, img_oth = _u8(img_own), _u8(img_oth)
        H, W = img_own.shape[:2]
        out = np.zeros((3, H - 2, W - 2, W - 2), np.float64)
        self._chk(self._lib.rsm_stage_refine_xi(self._h, _p(img_own), _p(img_oth), W, H, int(form), _p(out)))
        return out

    def div_unscaled(self, a, b):
        """(q_fast, q_ieee): the time-skewed refine kernel's division without operand scaling beside the device's a / b."""
        a = np.ascontiguousarray(a, np.float64).ravel()
        b = np.ascontiguousarray(b, np.float64).ravel()
        assert a.shape == b.shape
        qf = np.zeros(a.shape, np.float64)
        qi = np.zeros(a.shape, np.float64)
        self._chk(self._lib.rsm_stage_div_unscaled(self._h, _p(a), _p(b), a.size, _p(qf), _p(qi)))
        return qf, qi

    def sqrt_check(self, first_bits, n):
        """How many of the n floats with bit patterns first_bits .. first_bits + n - 1 the cloud filter's trimmed sqrtf gets wrong."""
        m = C.c_int64()
        self._chk(self._lib.rsm_stage_sqrt_check(self._h, int(first_bits), int(n), C.byref(m)))
        return int(m.value)

    def win_index_check(self, ncx, ncy):
        """How many candidates c < ncx * ncy of an ncx x ncy window the cloud filter's (row, column) split (csrc/win_index.h) gets
        wrong on the device, against the device's own c / ncx and c % ncx."""
        m = C.c_int64()
        self._chk(self._lib.rsm_stage_win_index_check(self._h, int(ncx), int(ncy), C.byref(m)))
        return int(m.value)

    def disparity_to_cloud(self, disp, mask_org, img_own, Q, scale, R, T, own, max_points=None):
        """(xyz, bgr) of DisparityToCloud.  max_points: the capacity handed to the stage (default W * H, which always
        holds the cloud); when given, returns (xyz, bgr, total): the whole capacity-sized host arrays, of which the stage
        fills the first min(total, max_points) records, and the number of points the cloud has."""
        d = np.ascontiguousarray(disp, np.float64); mask_org = _u8(mask_org); img_own = _u8(img_own)
        H, W = d.shape
        Q = np.ascontiguousarray(Q, np.float64); R = np.ascontiguousarray(R, np.float64)
        T = np.ascontiguousarray(T, np.float64)
        cap = W * H if max_points is None else int(max_points)
        xyz = np.zeros((cap, 3), np.float64); bgr = np.zeros((cap, 3), np.uint8)
        n = C.c_int64()
        self._chk(self._lib.rsm_stage_cloud(self._h, _p(d), _p(mask_org), _p(img_own), W, H, _p(Q), scale, _p(R), _p(T), C.byref(_bd(own)),
                                            _p(xyz), _p(bgr), cap, C.byref(n)))
        if max_points is not None:
            return xyz, bgr, int(n.value)
        return xyz[:n.value].copy(), bgr[:n.value].copy()
