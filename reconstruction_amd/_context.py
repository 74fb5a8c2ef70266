"""What every part of the binding shares (csrc/rsm_ctx.h's place on this side): page-locked host arrays, the small array helpers,
the context's lifetime / status check / options / profile, and the marshalling more than one subsystem needs."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Boundary, DedupView, RsmError


class _Pinned:
    """Owner of one rsm_host_alloc block (freed with the last array that views it)."""
    def __init__(self, nbytes):
        self._lib = _lib.load()
        self.ptr = self._lib.rsm_host_alloc(max(1, nbytes))
        if not self.ptr:
            raise RsmError(-3, "rsm_host_alloc(%d) failed" % nbytes)

    def __del__(self):
        try:
            self._lib.rsm_host_free(self.ptr)
        except Exception:
            pass


def host_empty(shape, dtype=np.float64):
    """numpy array in page-locked host memory (rsm_host_alloc): uploads from / downloads into it are single DMAs."""
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    own = _Pinned(n)
    buf = (C.c_uint8 * max(1, n)).from_address(own.ptr)
    buf._owner = own  # keeps the block alive as long as any view of `buf` lives
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def _host_buffer(shape, dtype, pinned, fill=None):
    """A result buffer, page-locked (host_empty) or pageable.  fill = None: zeroed lazily when pageable, as allocated when page-locked;
    a value: written now, so every page is touched before a timed call."""
    if not pinned:
        return np.zeros(shape, dtype) if fill is None else np.full(shape, fill, dtype)
    a = host_empty(shape, dtype)
    if fill is not None:
        a[...] = fill
    return a


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bd(t) -> Boundary:
    return t if isinstance(t, Boundary) else Boundary(*t)


def _normals4(normals, n):
    """[n,3] or [n,4] normals as the float32 [n,4] (nx, ny, nz, curvature) the library reads."""
    nrm = np.zeros((n, 4), np.float32)
    if n > 0:
        r = np.asarray(normals, np.float32).reshape(n, -1)
        nrm[:, :min(4, r.shape[1])] = r[:, :4]
    return nrm


def _views(cams, what, whole):
    """rsm_dedup_view per pair from cam[i][0..1].  whole: every view needs a mask, and the left view's bound and CamCenter are filled in
    (the duplicate deletion); otherwise a mask of None means all 255 and those two stay zero (the mesh colouring).  `what` names the caller
    in the error.  Returns (ctypes array, arrays to keep alive during the call)."""
    views = (DedupView * max(1, len(cams)))()
    keep = []
    for i, pair in enumerate(cams):
        v = views[i]
        shape = None
        for k in range(2):
            v.P[k][:] = np.asarray(pair[k].P, np.float64).reshape(3, 4).ravel().tolist()
            img = _u8(pair[k].image)
            msk = None if pair[k].mask is None and not whole else _u8(pair[k].mask)
            if img.ndim != 3 or img.shape[2] != 3 or (msk is not None and msk.shape != img.shape[:2]) or shape not in (None, img.shape[:2]):
                raise ValueError("%s: pair %d view %d: image %s / mask %s do not form one rectified pair" % (what, i, k, img.shape, None if msk is None else msk.shape))
            shape = img.shape[:2]
            keep += [img, msk]
            v.image[k], v.mask[k] = img.ctypes.data, (None if msk is None else msk.ctypes.data)
        if whole:
            v.cam_center[:] = np.asarray(pair[0].CamCenter, np.float32).ravel()[:3].tolist()
            v.bound0 = _bd(pair[0].bound)
        v.height, v.width = shape
    return views, keep


class ContextBase:
    """One rsm_ctx = one GPU. Not re-entrant (like CStereoMatching)."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        st = self._lib.rsm_create(C.byref(h), int(device))
        if st != 0:
            raise RsmError(st, "rsm_create(device=%d) failed -- is an MI355X visible? (no CPU fallback)" % device)
        self._h = h
        self.device = device
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rsm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, st):
        if st != 0:
            raise RsmError(st, (self._lib.rsm_last_error(self._h) or b"").decode())

    def set_option(self, name: str, value: int):
        self._chk(self._lib.rsm_set_option(self._h, name.encode(), value))

    # ---- measurement -----------------------------------------------------------------------------
    def profile_enable(self, on=True):
        """True / 1: events around every stage and every 8th launch of the dominant kernel; 2: the latter only."""
        self._chk(self._lib.rsm_profile_enable(self._h, int(on)))

    def profile_get(self):
        n = self._lib.rsm_profile_stage_count()
        ms, launches, byt = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_double * n)()
        self._chk(self._lib.rsm_profile_get(self._h, ms, launches, byt))
        return {self._lib.rsm_profile_stage_name(i).decode(): {"ms": ms[i], "launches": int(launches[i]), "bytes": byt[i]} for i in range(n)}
