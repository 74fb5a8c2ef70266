"""The pair path (csrc/rsm_api.hip): upload / rectify, run, download of one resident pair, and the loops over several pairs."""
import ctypes as C
import time
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._context import ContextBase, _host_buffer, _u8
from ._lib import PairIn, PairOut, RectifyIn, RectifyOut, RsmError


@dataclass
class PairResult:
    disparity: list            # [2] float64 HxW (NOMATCH = -10000)
    margin: list               # [2] (YL, YR, XL, XR, width, height)
    n_points: int
    xyz: np.ndarray            # n_points x 3 float64, InsertPoint order
    bgr: np.ndarray            # n_points x 3 uint8
    v_top: int


def _margins(pout):
    return [pout.margin[0].astuple(), pout.margin[1].astuple()]


class PairPart(ContextBase):
    @staticmethod
    def _pair_in(cfg, imgs=None, msks=None):
        pin = PairIn()
        imgs = imgs or [_u8(cfg.image[0]), _u8(cfg.image[1])]
        msks = msks or [_u8(cfg.mask[0]), _u8(cfg.mask[1])]
        H, W = msks[0].shape
        assert imgs[0].shape == (H, W, 3) and imgs[1].shape == (H, W, 3) and msks[1].shape == (H, W)
        assert (W, H) == (cfg.width, cfg.height)
        for v in range(2):
            pin.image[v] = imgs[v].ctypes.data
            pin.mask[v] = msks[v].ctypes.data
        pin.width, pin.height, pin.pyr_levels = W, H, cfg.pyr_levels
        pin.radius, pin.ws, pin.offset = cfg.radius, cfg.ws, cfg.offset
        pin.origin_width = cfg.origin_width or W
        pin.Q[:] = list(np.asarray(cfg.Q, np.float64).ravel())
        pin.R_final[:] = list(np.asarray(cfg.R_final, np.float64).ravel())
        pin.T_final[:] = list(np.asarray(cfg.T_final, np.float64).ravel())
        pin.verbose = int(getattr(cfg, "verbose", 0))
        return pin, (imgs, msks)

    def upload_pair(self, cfg):
        pin, keep = self._pair_in(cfg)
        self._chk(self._lib.rsm_upload_pair(self._h, C.byref(pin)))
        self._shape = (cfg.height, cfg.width)

    def upload_pair_device(self, cfg, image_ptrs, mask_ptrs):
        """image_ptrs / mask_ptrs: device addresses (e.g. torch.Tensor.data_ptr()) on this ctx's GPU."""
        pin, _ = self._pair_in(cfg)
        for v in range(2):
            pin.image[v] = int(image_ptrs[v])
            pin.mask[v] = int(mask_ptrs[v])
        self._chk(self._lib.rsm_upload_pair_device(self._h, C.byref(pin)))
        self._shape = (cfg.height, cfg.width)

    def rectify_pair(self, K, E, origin_size, lowest_size, pyr_levels, images, masks, radius=2, ws=0.03, offset=2, verbose=0, want_images=True):
        """CStereoMatching::Rectify for one pair on the GPU (.cpp:117-168); the rectified pair stays resident, so
        run_pair() can follow.  K / E: [2] 3x3 / 3x4, images / masks: raw BGR / grey arrays of origin size
        (width, height).  Returns dict(image, mask, Q, R_final, T_final, P, size)."""
        rin, rout = RectifyIn(), RectifyOut()
        imgs = [_u8(i) for i in images]
        msks = [_u8(m) for m in masks]
        ow, oh = int(origin_size[0]), int(origin_size[1])
        for v in range(2):
            assert imgs[v].shape == (oh, ow, 3) and msks[v].shape == (oh, ow)
            rin.K[v][:] = list(np.asarray(K[v], np.float64).ravel())
            rin.E[v][:] = list(np.asarray(E[v], np.float64).ravel())
            rin.image[v] = imgs[v].ctypes.data
            rin.mask[v] = msks[v].ctypes.data
        rin.origin_width, rin.origin_height = ow, oh
        rin.lowest_width, rin.lowest_height, rin.pyr_levels = int(lowest_size[0]), int(lowest_size[1]), int(pyr_levels)
        W, H = rin.lowest_width << (pyr_levels - 1), rin.lowest_height << (pyr_levels - 1)
        rimg = [np.zeros((H, W, 3), np.uint8) for _ in range(2)] if want_images else [None, None]
        rmsk = [np.zeros((H, W), np.uint8) for _ in range(2)] if want_images else [None, None]
        if want_images:
            for v in range(2):
                rout.image[v] = rimg[v].ctypes.data
                rout.mask[v] = rmsk[v].ctypes.data
        self._chk(self._lib.rsm_rectify_pair(self._h, C.byref(rin), int(radius), ws, int(offset), int(verbose), C.byref(rout)))
        self._shape = (H, W)
        return dict(image=rimg, mask=rmsk, Q=np.array(rout.Q).reshape(4, 4), R_final=np.array(rout.R_final).reshape(3, 3),
                    T_final=np.array(rout.T_final), P=[np.array(rout.P[v]).reshape(3, 4) for v in range(2)], size=(W, H))

    def run_pair(self):
        self._chk(self._lib.rsm_run_pair(self._h))

    def _new_result(self, cap, pinned, cloud_pinned, want_disparity) -> PairResult:
        """An empty PairResult over fresh buffers: two HxW maps when wanted, xyz / bgr of capacity `cap` points."""
        H, W = self._shape
        d = [_host_buffer((H, W), np.float64, pinned) for _ in range(2)] if want_disparity else [None, None]
        xyz_buf, bgr_buf = _host_buffer((cap, 3), np.float64, cloud_pinned), _host_buffer((cap, 3), np.uint8, cloud_pinned)
        res = PairResult(disparity=d, margin=[None, None], n_points=0, xyz=xyz_buf[:0], bgr=bgr_buf[:0], v_top=0)
        res._xyz_buf, res._bgr_buf = xyz_buf, bgr_buf
        return res

    def alloc_result(self, pinned=False, want_cloud=True, want_disparity=True) -> PairResult:
        """Result buffers for download_pair(into=...) sized for ANY cloud of the resident pair's size (W*H points: the
        point count depends on the data), page-locked when `pinned`."""
        H, W = self._shape
        return self._new_result(W * H if want_cloud else 0, pinned, pinned, want_disparity)

    def download_pair(self, want_cloud=True, want_disparity=True, pinned=False, into=None) -> PairResult:
        """pinned: the results land in page-locked arrays (host_empty) instead of pageable ones; into: a PairResult whose
        buffers are reused (no allocation) -- one from alloc_result() (capacity W*H points: fits every cloud) or from an
        earlier download (capacity = that cloud's size; a larger cloud raises RsmError, nothing is truncated).  n_points,
        v_top, margin and the xyz / bgr views of `into` are refreshed from this download."""
        H, W = self._shape
        if into is None:   # a call without buffers learns n_points; the buffers then hold exactly that many
            pout = PairOut()
            self._chk(self._lib.rsm_download_pair(self._h, C.byref(pout)))
            into = self._new_result(int(pout.n_points), pinned, pinned and want_cloud, want_disparity)
            into.xyz, into.bgr = into._xyz_buf, into._bgr_buf   # (without want_cloud: n_points rows of zeros)
        xyz_buf = getattr(into, "_xyz_buf", None)
        bgr_buf = getattr(into, "_bgr_buf", None)
        if xyz_buf is None:
            xyz_buf, bgr_buf = into.xyz, into.bgr
        pout = PairOut()
        if want_disparity:
            for v in range(2):
                dv = into.disparity[v]
                if dv is None or dv.shape != (H, W) or dv.dtype != np.float64 or not dv.flags.c_contiguous:
                    raise RsmError(-1, "download_pair(into=): disparity[%d] must be a C-contiguous float64 %dx%d array" % (v, H, W))
                pout.disparity[v] = dv.ctypes.data
        cap = int(xyz_buf.shape[0]) if want_cloud else 0
        if want_cloud:
            if bgr_buf.shape[0] != cap or xyz_buf.dtype != np.float64 or bgr_buf.dtype != np.uint8:
                raise RsmError(-1, "download_pair(into=): xyz / bgr buffers disagree")
            pout.max_points = cap
            pout.xyz = xyz_buf.ctypes.data if cap else None
            pout.bgr = bgr_buf.ctypes.data if cap else None
        self._chk(self._lib.rsm_download_pair(self._h, C.byref(pout)))
        n = int(pout.n_points)
        if want_cloud and n > cap:
            raise RsmError(-1, "download_pair(into=): the cloud has %d points, the buffers hold %d (use Context.alloc_result())" % (n, cap))
        into.n_points, into.v_top = n, int(pout.v_top)
        into.margin = _margins(pout)
        if want_cloud:
            into._xyz_buf, into._bgr_buf = xyz_buf, bgr_buf
            into.xyz, into.bgr = xyz_buf[:n], bgr_buf[:n]
        return into

    POINT16 = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("b", np.uint8), ("g", np.uint8), ("r", np.uint8), ("pad", np.uint8)])

    def download_points16(self, pinned=False) -> np.ndarray:
        """The last cloud as rsm_point16 records (float xyz = InsertPoint's cast, CCloudOptimization.cpp:61, + BGR), packed on
        the GPU and downloaded through rsm_pair_out.points16: a structured array of n_points records."""
        n = self.n_points
        rec = _host_buffer((max(n, 1),), self.POINT16, pinned)
        pout = PairOut()
        pout.max_points = n
        pout.points16 = rec.ctypes.data
        self._chk(self._lib.rsm_download_pair(self._h, C.byref(pout)))
        return rec[:n]

    def match_pair(self, cfg, want_cloud=True) -> PairResult:
        self.upload_pair(cfg)
        self.run_pair()
        return self.download_pair(want_cloud=want_cloud)

    def result_device(self):
        """(disparity0_ptr, disparity1_ptr, n_points, xyz_ptr, bgr_ptr) device addresses of the last run."""
        d0, d1, xyz, bgr = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = C.c_int64()
        self._chk(self._lib.rsm_result_device(self._h, C.byref(d0), C.byref(d1), C.byref(n), C.byref(xyz), C.byref(bgr)))
        return d0.value, d1.value, int(n.value), xyz.value, bgr.value

    @property
    def n_points(self):
        return self.result_device()[2]

    def export_cloud_device(self, xyz_ptr, bgr_ptr, max_points):
        """D2D copy of the last cloud into caller-owned device buffers (addresses, e.g. tensor.data_ptr())."""
        self._chk(self._lib.rsm_export_cloud_device(self._h, xyz_ptr, bgr_ptr, max_points))

    def pack_cloud16(self, dst_ptr, max_points) -> int:
        """rsm_pack_cloud16: the last cloud as 16-byte point records (float xyz + BGR) into a caller-owned device
        buffer (address); returns the number of records written."""
        n = C.c_int64()
        self._chk(self._lib.rsm_pack_cloud16(self._h, dst_ptr, max_points, C.byref(n)))
        return int(n.value)


def _handles(ctxs):
    return (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])


def run_pairs(ctxs, repeats=1):
    """rsm_run_pairs[_repeat]: rsm_run_pair on several DIFFERENT contexts concurrently (pairs already resident),
    each context `repeats` times back to back."""
    lib = _lib.load()
    st = lib.rsm_run_pairs_repeat(_handles(ctxs), len(ctxs), int(repeats))
    if st != 0:
        msgs = [(lib.rsm_last_error(c._h) or b"").decode() for c in ctxs]
        raise RsmError(st, "; ".join(m for m in msgs if m))


def _pairs_io(cfgs, want_cloud, want_disparity, pinned):
    """rsm_pair_in / rsm_pair_out arrays + the host buffers behind them for a list of pair configs."""
    n = len(cfgs)
    ins = (PairIn * max(n, 1))()
    outs = (PairOut * max(n, 1))()
    keep, bufs = [], []
    for p, cfg in enumerate(cfgs):
        pin, k = PairPart._pair_in(cfg)
        ins[p] = pin
        keep.append(k)
        H, W = cfg.height, cfg.width
        d = [_host_buffer((H, W), np.float64, pinned, 0.0) for _ in range(2)] if want_disparity else [None, None]   # filled: pages touched now
        xyz = _host_buffer((W * H, 3), np.float64, pinned, 0.0) if want_cloud else None
        bgr = _host_buffer((W * H, 3), np.uint8, pinned, 0) if want_cloud else None
        if want_disparity:
            outs[p].disparity[0] = d[0].ctypes.data
            outs[p].disparity[1] = d[1].ctypes.data
        if want_cloud:
            outs[p].max_points = W * H
            outs[p].xyz = xyz.ctypes.data
            outs[p].bgr = bgr.ctypes.data
        bufs.append((d, xyz, bgr))
    return ins, outs, keep, bufs


def _pairs_results(n, outs, bufs, status, want_cloud):
    res = []
    for p in range(n):
        if status[p] != 0:
            res.append(None)
            continue
        d, xyz, bgr = bufs[p]
        m = int(outs[p].n_points)
        res.append(PairResult(disparity=d, margin=_margins(outs[p]), n_points=m, xyz=xyz[:m] if want_cloud else np.zeros((0, 3)),
                              bgr=bgr[:m] if want_cloud else np.zeros((0, 3), np.uint8), v_top=int(outs[p].v_top)))
    return res


def match_pairs(ctxs, cfgs, want_cloud=True, want_disparity=True, timing=None, pinned=False):
    """rsm_match_pairs: the pair loop of MatchAllLayer (.cpp:17-33) for a list of pair configs over a pool of
    contexts (same or different GPUs), pairs in flight together.  Returns (results in pair order, statuses).
    timing (optional dict) receives "call_s": seconds inside the C call alone (output buffers pre-faulted, the
    slicing of the results outside).  pinned: the output buffers are page-locked (host_empty)."""
    lib = _lib.load()
    n = len(cfgs)
    ins, outs, keep, bufs = _pairs_io(cfgs, want_cloud, want_disparity, pinned)
    status = (C.c_int * max(n, 1))()
    arr = _handles(ctxs)
    t0 = time.perf_counter()
    lib.rsm_match_pairs(arr, len(ctxs), ins, outs, n, status)
    if timing is not None:
        timing["call_s"] = time.perf_counter() - t0
    return _pairs_results(n, outs, bufs, status, want_cloud), list(status)[:n]


def match_pairs_multi_gpu(cfgs, n_gpus=0, pairs_in_flight=2, want_cloud=True, want_disparity=True):
    """rsm_match_pairs_multi_gpu: the same loop sharded over the GPUs of this node from ONE process; the
    library creates and destroys its own contexts (context i on GPU i % n_gpus, `pairs_in_flight` per GPU).
    n_gpus = 0: every visible GPU.  Returns (results in pair order -- None for a failed pair --, statuses, return code)."""
    lib = _lib.load()
    n = len(cfgs)
    ins, outs, keep, bufs = _pairs_io(cfgs, want_cloud, want_disparity, False)
    status = (C.c_int * max(n, 1))()
    rc = lib.rsm_match_pairs_multi_gpu(ins, n, int(n_gpus), int(pairs_in_flight), outs, status)
    return _pairs_results(n, outs, bufs, status, want_cloud), list(status)[:n], int(rc)
