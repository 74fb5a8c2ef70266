"""The cloud stages after the pair path (csrc/rsm_cloud.hip): the per-pair filter, MLS smoothing, multi-view duplicate deletion."""
import ctypes as C

import numpy as np

from ._context import ContextBase, _bd, _normals4, _p, _u8, _views
from ._lib import FilterParams, MlsParams, OutremParams


class CloudPart(ContextBase):
    # ---- per-pair cloud filter (CCloudOptimization::filter, CloudOptimization/CCloudOptimization.cpp:82-121) ----
    def _filter(self, fn, before, after, mean_k, std_mul, normal_radius, cam_center):
        """One of the three rsm_filter_* entries, its arguments before / after the parameters: (n_kept, stats dict)."""
        prm = FilterParams(int(mean_k), float(std_mul), float(normal_radius))
        prm.cam_center[:] = [float(v) for v in np.asarray(cam_center, np.float64).ravel()[:3]]
        m, st = C.c_int64(), (C.c_double * 4)()
        self._chk(fn(self._h, *before, C.byref(prm), *after, C.byref(m), st))
        return int(m.value), dict(mean=st[0], stddev=st[1], threshold=st[2], exhaustive=int(st[3]))

    def filter_cloud(self, xyz, mean_k=100, std_mul=1.0, normal_radius=2.5, cam_center=(0.0, 0.0, 0.0)):
        """StatisticalOutlierRemoval + radius-search normals turned toward cam_center on a host cloud (n x 3, cast to
        float32 as InsertPoint does).  Returns (kept_index int32 [m], normals float32 [m,4] = nx, ny, nz, curvature,
        stats dict)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        kept = np.zeros(max(n, 1), np.int32)
        nrm = np.zeros((max(n, 1), 4), np.float32)
        m, stats = self._filter(self._lib.rsm_filter_cloud, (_p(xyz), n), (_p(kept), _p(nrm)), mean_k, std_mul, normal_radius, cam_center)
        return kept[:m].copy(), nrm[:m].copy(), stats

    def filter_last_cloud(self, points_ptr, normals_ptr, max_points, mean_k=100, std_mul=1.0, normal_radius=2.5,
                          cam_center=(0.0, 0.0, 0.0)):
        """The same on the last run's cloud without leaving the GPU: surviving points as 16-byte records and their
        normals into caller-owned device buffers (addresses).  Returns (n_kept, stats dict)."""
        return self._filter(self._lib.rsm_filter_last_cloud, (), (points_ptr, normals_ptr, max_points), mean_k, std_mul, normal_radius, cam_center)

    def filter_last_cloud_host(self, mean_k=100, std_mul=1.0, normal_radius=2.5, cam_center=(0.0, 0.0, 0.0), want_normals=True):
        """rsm_filter_last_cloud_host: the per-pair filter on the GPU, its output -- the surviving points as rsm_point16 records
        and their oriented normals (nx, ny, nz, curvature) -- downloaded.  Returns (records, normals or None, stats dict)."""
        n = self.n_points
        rec = np.zeros(max(n, 1), self.POINT16)
        nrm = np.zeros((max(n, 1), 4), np.float32) if want_normals else None
        k, stats = self._filter(self._lib.rsm_filter_last_cloud_host, (), (_p(rec), _p(nrm) if want_normals else None, n), mean_k, std_mul, normal_radius,
                                cam_center)
        return rec[:k], (nrm[:k] if want_normals else None), stats

    def filter_last_info(self) -> dict:
        """What the last filter_last_cloud[_host] did: whether the pixel-window pass ran, how many queries it left to the grid search."""
        v = (C.c_int64 * 4)()
        self._chk(self._lib.rsm_filter_last_info(self._h, v))
        w = (C.c_int64 * 2)()
        self._chk(self._lib.rsm_filter_last_normals_info(self._h, w))
        return dict(window=bool(v[0]), radius=int(v[0]), undecided=int(v[1]), points=int(v[2]), kept=int(v[3]), normals_window=int(w[0]), normals_need=int(w[1]))

    def filter_depth_map(self, disp, mask_org, img_own, Q, scale, R, T, own, mean_k=100, std_mul=1.0, normal_radius=2.5, cam_center=(0.0, 0.0, 0.0),
                         max_points=None):
        """rsm_stage_filter_depth_map: DisparityToCloud of a top-level fp64 disparity map, then the per-pair filter of that cloud as
        filter_last_cloud runs it (same options, same filter_last_* reports) -- no matching.  Returns (xyz float32 [n,3]: the unfiltered
        cloud, kept_index int32 [m], normals float32 [m,4], stats dict)."""
        d = np.ascontiguousarray(disp, np.float64); mask_org = _u8(mask_org); img_own = _u8(img_own)
        H, W = d.shape
        Q, R, T = (np.ascontiguousarray(a, np.float64) for a in (Q, R, T))
        cap = W * H if max_points is None else int(max_points)
        xyz = np.zeros((max(cap, 1), 3), np.float32)
        kept = np.zeros(max(cap, 1), np.int32)
        nrm = np.zeros((max(cap, 1), 4), np.float32)
        n = C.c_int64()
        m, stats = self._filter(self._lib.rsm_stage_filter_depth_map, (_p(d), _p(mask_org), _p(img_own), W, H, _p(Q), float(scale), _p(R), _p(T), C.byref(_bd(own))),
                                (_p(xyz), _p(kept), _p(nrm), cap, C.byref(n)), mean_k, std_mul, normal_radius, cam_center)
        return xyz[:n.value].copy(), kept[:m].copy(), nrm[:m].copy(), stats

    def filter_last_passes(self) -> dict:
        """The passes between the tile pass and the grid ladder of the last filter_last_cloud[_host] / filter_depth_map
        (rsm_filter_last_passes): `passes` = one dict per pass that ran a wave or a workgroup per query (radius, entered, decided,
        workgroup), `ladder` / `whole` = the queries handed to the grid ladder / the whole-cloud search, `whole_over_lattice` = whether
        that search read the lattice copy."""
        head, cnt = (C.c_int64 * 4)(), C.c_int64()
        self._chk(self._lib.rsm_filter_last_passes(self._h, head, None, 0, C.byref(cnt)))
        rows = (C.c_int64 * (4 * max(int(head[3]), 1)))()
        self._chk(self._lib.rsm_filter_last_passes(self._h, head, rows, int(head[3]), C.byref(cnt)))
        passes = [dict(radius=int(rows[4 * i]), entered=int(rows[4 * i + 1]), decided=int(rows[4 * i + 2]), workgroup=bool(rows[4 * i + 3]))
                  for i in range(int(cnt.value))]
        return dict(passes=passes, ladder=int(head[0]), whole=int(head[1]), whole_over_lattice=bool(head[2]))

    def filter_last_grid(self) -> dict:
        """The k-nearest grid ladder of the last filter_cloud / filter_last_cloud[_host]: its first level's search radius h (float32),
        grid origin and cells per world axis, the levels run and the cell-table kinds they searched with (option "filter_ladder_h")."""
        g = (C.c_double * 4)()
        v = (C.c_int64 * 6)()
        self._chk(self._lib.rsm_filter_last_grid(self._h, g, v))
        return dict(h=np.float32(g[0]), origin=np.array(g[1:4], np.float32), cells=[int(v[a]) for a in range(3)], levels=int(v[3]),
                    kind0=int(v[4]), kinds=sorted(t for t in range(3) if (v[5] >> t) & 1))

    # ---- the radius outlier pass behind the outlier removal (pcl::RadiusOutlierRemoval, CCloudOptimization.cpp:90-96) ----
    def set_filter_outrem(self, min_neighbors=None, radius=None):
        """rsm_filter_set_outrem: from now on every filter_* entry of this context removes, after the StatisticalOutlierRemoval, the
        survivors with at most min_neighbors finite survivors (themselves included) within radius, and computes the normals on what is
        left.  Both None: off (the default).  RsmError names what the library refuses (a negative count, a radius that is not positive and
        finite in float32)."""
        if min_neighbors is None and radius is None:
            self._chk(self._lib.rsm_filter_set_outrem(self._h, None))
            return
        if min_neighbors is None or radius is None:
            raise ValueError("set_filter_outrem: min_neighbors and radius go together (both None switches the pass off)")
        prm = OutremParams(int(min_neighbors), float(radius))
        self._chk(self._lib.rsm_filter_set_outrem(self._h, C.byref(prm)))

    def filter_last_outrem(self) -> dict:
        """What that pass did in the last filter call (rsm_filter_last_outrem): points_in (-1: the pass was off), removed, window (the
        pixel window of the lattice route, 0 = the grid route), nonfinite (non-finite points among the removed)."""
        v = (C.c_int64 * 4)()
        self._chk(self._lib.rsm_filter_last_outrem(self._h, v))
        return dict(points_in=int(v[0]), removed=int(v[1]), window=int(v[2]), nonfinite=int(v[3]))

    def radius_count(self, xyz, radius, cap=None):
        """rsm_stage_radius_count: per point of a host cloud (n x 3, float32) the finite points with float32 squared distance below
        (float)(radius * radius), itself included, counted up to cap (None: the full count).  Returns int32 [n]."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        cnt = np.zeros(max(n, 1), np.int32)
        self._chk(self._lib.rsm_stage_radius_count(self._h, _p(xyz), n, float(radius), 2 ** 31 - 1 if cap is None else int(cap), _p(cnt)))
        return cnt[:n].copy()

    # ---- moving-least-squares smoothing (CCloudOptimization::run, CloudOptimization/CCloudOptimization.cpp:348-389) ----
    def mls_cloud(self, xyz, radius=2.5, order=1, ref_normals=None):
        """pcl::MovingLeastSquares (normals on, polynomial `order`, no upsampling) on a host cloud (n x 3, float32); with
        ref_normals ([n,4] or [n,3]: the filter's normals) each output normal is negated where it disagrees with its
        input point's (.cpp:378-385).  Returns (xyz float32 [m,3], normals float32 [m,4] = nx, ny, nz, curvature,
        src_index int32 [m]) in input order."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        ref = None if ref_normals is None else _normals4(ref_normals, n)
        oxyz = np.zeros((max(n, 1), 3), np.float32)
        onrm = np.zeros((max(n, 1), 4), np.float32)
        oidx = np.zeros(max(n, 1), np.int32)
        m = C.c_int64()
        prm = MlsParams(float(radius), int(order))
        self._chk(self._lib.rsm_mls_cloud(self._h, _p(xyz), n, None if ref is None else _p(ref), C.byref(prm), _p(oxyz), _p(onrm), _p(oidx), C.byref(m)))
        k = int(m.value)
        return oxyz[:k].copy(), onrm[:k].copy(), oidx[:k].copy()

    def mls_cloud_device(self, points_ptr, n, ref_normals_ptr, out_xyz_ptr, out_normals_ptr, src_index_ptr, radius=2.5, order=1):
        """rsm_mls_cloud_device on device buffers (addresses): n rsm_point16 records in, n float4 reference normals (or 0 / None:
        no flip); outputs of capacity n.  Returns the number of points emitted."""
        m = C.c_int64()
        prm = MlsParams(float(radius), int(order))
        self._chk(self._lib.rsm_mls_cloud_device(self._h, points_ptr, n, ref_normals_ptr, C.byref(prm), out_xyz_ptr, out_normals_ptr, src_index_ptr, C.byref(m)))
        return int(m.value)

    # ---- multi-view duplicate deletion (CCloudOptimization::run's isdelete branch, CloudOptimization/CCloudOptimization.cpp:152-346) ----
    @staticmethod
    def dedup_views(cams):
        """rsm_dedup_view per pair from cam[i][0..1] (Camera objects: P, image, mask, CamCenter, and bound on the left view, as
        Rectify and MatchAllLayer leave them).  Returns (ctypes array, arrays to keep alive during the call)."""
        return _views(cams, "dedup", True)

    def _dedup(self, fn, before, cams, after):
        """One of the two rsm_dedup_cloud* entries, its arguments before / after the views: (m, stats dict)."""
        views, keep = self.dedup_views(cams)
        m, st = C.c_int64(), (C.c_int64 * 4)()
        self._chk(fn(self._h, *before, views, len(cams), *after, C.byref(m), st))
        del keep
        return int(m.value), dict(s1=int(st[0]), s2=int(st[1]), count0=int(st[2]), visited=int(st[3]))

    def dedup_cloud(self, xyz, normals, cams):
        """The isdelete branch on a host cloud: xyz [n,3] float32 and the filter's normals [n,4] (or [n,3]) of the pairs' filtered
        clouds in pair order, cams = m_ImageData.cam.  Returns (indicesptr int32 [m], stats dict s1 / s2 / count0 / visited)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        nrm = _normals4(normals, n)
        idx = np.zeros(max(n, 1), np.int32)
        m, stats = self._dedup(self._lib.rsm_dedup_cloud, (_p(xyz), _p(nrm), n), cams, (_p(idx),))
        return idx[:m].copy(), stats

    def dedup_cloud_device(self, points_ptr, normals_ptr, n, cams, index_ptr, out_points_ptr=None, out_normals_ptr=None):
        """rsm_dedup_cloud_device on device buffers (addresses): n rsm_point16 records and n float4 normals in; indicesptr (capacity
        n) and, when given, the kept records / normals out.  Returns (m, stats dict)."""
        return self._dedup(self._lib.rsm_dedup_cloud_device, (points_ptr, normals_ptr, n), cams, (index_ptr, out_points_ptr, out_normals_ptr))
