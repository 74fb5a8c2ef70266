"""Host-side mirror of the reference's call surface for the CStereoMatching path.

`StereoMatching` keeps the names, argument meaning and error behaviour of
reconstruction/CStereoMatching.h:35-48 (Init / MatchAllLayer, public fields Q, R_final, T_final,
margin, MatchBlockRadius, m_ws, m_offset, Verbose); `ManageData` / `Camera` carry the fields of
CManageData.h:16-40 this path reads and writes.  All compute goes through the C ABI of
include/rsm.h (librsm_mi355.so, hand-written HIP for gfx950) -- there is no CPU path here.

MatAllLayer either rectifies on the GPU (cameras carry calibration + raw image / mask
files or arrays, `ManageData.rectified[pair]` is absent) or starts from rectified inputs (each
`ManageData.cam[pair][v]` holds what Rectify leaves in `.image` / `.mask`, .cpp:154-158, and
`ManageData.rectified[pair]` the Q / R_final / T_final it computes, .cpp:128-138).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._cloud import CloudPart
from ._context import _Pinned, _bd, _p, _u8, host_empty  # noqa: F401
from ._lib import Boundary, DedupView, FilterParams, MeshCleanParams, MeshColorParams, MlsParams, PoissonParams, NOMATCH, PairIn, PairOut, RectifyIn, RectifyOut, RsmError  # noqa: F401
from ._mesh import POISSON_BAND_MAX_ITERATIONS, POISSON_MAX_CYCLES, POISSON_REL_RESIDUAL, MeshPart
from ._pair import PairPart, PairResult, match_pairs, match_pairs_multi_gpu, run_pairs  # noqa: F401
from ._stages import StagesPart


class Context(PairPart, StagesPart, CloudPart, MeshPart):
    """One rsm_ctx = one GPU. Not re-entrant (like CStereoMatching).  The parts follow the host library's units: the pair path (_pair.py,
    csrc/rsm_api.hip), the parity stages (_stages.py), the cloud (_cloud.py) and the mesh (_mesh.py); _context.py holds what they share."""


def stereo_rectify(K1, K2, size, R, T):
    """cv::stereoRectify(K1, 0, K2, 0, size, R, T, flags=0, alpha=-1) through the C ABI (host fp64, no GPU needed)."""
    a = [np.ascontiguousarray(x, np.float64) for x in (K1, K2, R, T)]
    R1 = np.zeros((3, 3)); R2 = np.zeros((3, 3)); P1 = np.zeros((3, 4)); P2 = np.zeros((3, 4)); Q = np.zeros((4, 4))
    st = _lib.load().rsm_stereo_rectify(_p(a[0]), _p(a[1]), int(size[0]), int(size[1]), _p(a[2]), _p(a[3]),
                                        _p(R1), _p(R2), _p(P1), _p(P2), _p(Q))
    if st != 0:
        raise RsmError(st, "rsm_stereo_rectify")
    return R1, R2, P1, P2, Q


def write_ply(path, xyz, bgr, normals=None):
    """cloud%d.ply of DisparityToCloud (.cpp:723-729,754-756) through the C ABI (host-only, no GPU needed).
    With `normals` ([n,4]: nx, ny, nz, curvature -- pcl::PointNormal's fields, what filter() accumulates in
    cloud_normals, CCloudOptimization.cpp:123) the same records are followed by four float properties."""
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    bgr = _u8(bgr).reshape(-1, 3)
    assert len(xyz) == len(bgr)
    if normals is not None:
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 4)
        assert len(nrm) == len(xyz)
        rec = np.zeros(len(xyz), dtype=[("xyz", "<f4", 3), ("bgr", "u1", 3), ("n", "<f4", 4)])
        rec["xyz"], rec["bgr"], rec["n"] = xyz.astype(np.float32), bgr, nrm
        with open(path, "wb") as f:
            f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                     "property float z\nproperty uchar blue\nproperty uchar green\nproperty uchar red\nproperty float nx\n"
                     "property float ny\nproperty float nz\nproperty float curvature\nend_header\n" % len(xyz)).encode())
            f.write(rec.tobytes())
        return
    st = _lib.load().rsm_write_ply(str(path).encode(), _p(xyz), _p(bgr), len(xyz))
    if st != 0:
        raise RsmError(st, "rsm_write_ply(%s)" % path)


def write_ply_pointnormal(path, xyz, normals):
    """tmp\\bigcloud.ply of CCloudOptimization::run (CCloudOptimization.cpp:389): pcl::io::savePLYFileBinary of a
    pcl::PointCloud<pcl::PointNormal> -- binary little-endian, float x y z normal_x normal_y normal_z curvature per vertex.
    normals: [n,4] (nx, ny, nz, curvature) as mls_cloud returns them.  Host-only."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 4)
    assert len(xyz) == len(nrm)
    rec = np.empty((len(xyz), 7), "<f4")
    rec[:, :3], rec[:, 3:] = xyz, nrm
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float normal_x\nproperty float normal_y\nproperty float normal_z\nproperty float curvature\nend_header\n"
                 % len(xyz)).encode())
        f.write(rec.tobytes())


def write_ply_mesh(path, vertices, faces, rgb=None):
    """The mesh as a binary little-endian PLY (vertex float x y z, face list uchar int vertex_indices: what MeshLab and TextureStitcher
    read) through the C ABI (rsm_write_ply_mesh; host-only, no GPU needed).  With rgb (uint8 [nv,3]: red, green, blue) every vertex also
    carries uchar red green blue, MyPlyIo's property order (my_ply_interface.cpp:35-50; rsm_write_ply_mesh_color)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    if rgb is not None:
        c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError("write_ply_mesh: %d colours for %d vertices" % (len(c), len(v)))
        st = _lib.load().rsm_write_ply_mesh_color(str(path).encode(), _p(v), len(v), _p(f), len(f), _p(c))
        if st != 0:
            raise RsmError(st, "rsm_write_ply_mesh_color(%s)" % path)
        return
    st = _lib.load().rsm_write_ply_mesh(str(path).encode(), _p(v), len(v), _p(f), len(f))
    if st != 0:
        raise RsmError(st, "rsm_write_ply_mesh(%s)" % path)



# ---------------------------------------------------------------------------------------------------
# Mirror of the reference's data / matching classes
# ---------------------------------------------------------------------------------------------------
@dataclass
class Camera:
    """struct camera (CManageData.h:16-26), the fields this path touches."""
    camID: int = 0
    image: np.ndarray | None = None   # rectified top-level BGR (what Rectify stores, .cpp:154)
    mask: np.ndarray | None = None    # rectified + eroded mask (.cpp:156-158)
    P: np.ndarray | None = None       # 3x4 projection (.cpp:143-145), carried through untouched
    bound: tuple | None = None        # written by MatchAllLayer (.cpp:27-28)
    image_name: str = ""
    mask_name: str = ""
    MatIntrinsics: np.ndarray | None = None   # 3x3 (CManageData.cpp:59)
    MatExtrinsics: np.ndarray | None = None   # 3x4 (CManageData.cpp:60)
    CamCenter: np.ndarray | None = None       # -R^T t as float32 (CManageData.cpp:61-62)


@dataclass
class ManageData:
    """CManageData (CManageData.h:28-61), the members MatchAllLayer reads."""
    cam: list = field(default_factory=list)          # cam[pair][0..1] -> Camera
    m_PyrmNum: int = 4
    m_LowestLevelSize: tuple = (160, 240)            # (width, height)
    m_OriginSize: tuple = (0, 0)                     # (width, height)
    isoutput: int = 0
    rectified: list = field(default_factory=list)    # per pair: dict(Q=4x4, R_final=3x3, T_final=3)

    @property
    def m_CampairNum(self):
        return len(self.cam)


class _PairCfg:
    pass


class StereoMatching:
    """CStereoMatching (CStereoMatching.h:35-71) on MI355X.

    Init(data, CloudOptimization, radii=2, ws=0.5, disparity_offset=2) and MatchAllLayer() keep the
    reference's signatures; per point `CloudOptimization.InsertPoint(point3)` is called in the
    reference's row-major order (or `InsertPoints(xyz)` once per pair when the sink offers it),
    then `CloudOptimization.filter(CamPair)` (.cpp:29-31).
    """

    def __init__(self, device: int = 0):
        self._ctx = Context(device)
        self.m_data = None
        self.m_CloudOptimization = None
        self.MatchBlockRadius = 2
        self.m_ws = 0.5
        self.m_offset = 2
        self.Q = None
        self.R_final = None
        self.T_final = None
        self.margin = [None, None]
        self.Verbose = 1
        self.disparity = [None, None]   # last pair's fp64 disparity maps (the reference keeps them local)

    def Init(self, data, CloudOptimization=None, radii=2, ws=0.5, disparity_offset=2):
        self.m_data = data
        self.m_CloudOptimization = CloudOptimization
        self.MatchBlockRadius = radii
        self.m_ws = ws
        self.m_offset = disparity_offset
        self.Verbose = 1

    def MatchAllLayer(self):
        data = self.m_data
        top = 1 << (data.m_PyrmNum - 1)
        W, H = data.m_LowestLevelSize[0] * top, data.m_LowestLevelSize[1] * top  # .cpp:120
        for CamPair in range(data.m_CampairNum):
            cams = data.cam[CamPair]
            if self.Verbose >= 1:
                print("processing pair %d: cam %d and cam %d..." % (CamPair + 1, cams[0].camID, cams[1].camID))
            pre_rectified = CamPair < len(data.rectified) and data.rectified[CamPair] is not None
            if not pre_rectified:
                # Rectify(CamPair, Q), .cpp:20 / :117-168: raw images + calibration -> rectified pair on the GPU
                from . import config as _cfg
                if self.Verbose >= 1:
                    print("\trectifying...")
                raw, rawm = [], []
                for j in range(2):
                    img = getattr(cams[j], "raw_image", None)
                    if img is None:
                        img = _cfg.imread_bgr(cams[j].image_name)
                    if img is None:
                        print("read image %s error" % cams[j].image_name)   # .cpp:147-151: silent return
                        return
                    msk = getattr(cams[j], "raw_mask", None)
                    if msk is None:
                        msk = _cfg.imread_gray(cams[j].mask_name)
                    if msk is None:
                        print("read image %s error" % cams[j].mask_name)
                        return
                    raw.append(img)
                    rawm.append(msk)
                rect = self._ctx.rectify_pair([cams[0].MatIntrinsics, cams[1].MatIntrinsics],
                                              [cams[0].MatExtrinsics, cams[1].MatExtrinsics], data.m_OriginSize,
                                              data.m_LowestLevelSize, data.m_PyrmNum, raw, rawm)
                for j in range(2):
                    cams[j].image, cams[j].mask, cams[j].P = rect["image"][j], rect["mask"][j], rect["P"][j]
                    if getattr(data, "isoutput", 0):   # .cpp:159-166: "%d_%d.jpg" of the rectified image
                        _cfg.imwrite_bgr("%d_%d.jpg" % (CamPair, cams[j].camID), cams[j].image)
            else:
                if cams[0].image is None or cams[1].image is None:
                    print("read image %s error" % (cams[0].image_name or cams[1].image_name))
                    return
                rect = data.rectified[CamPair]
            self.Q = np.asarray(rect["Q"], np.float64)
            self.R_final = np.asarray(rect["R_final"], np.float64)
            self.T_final = np.asarray(rect["T_final"], np.float64)
            cfg = _PairCfg()
            cfg.width, cfg.height, cfg.pyr_levels = W, H, data.m_PyrmNum
            cfg.radius, cfg.ws, cfg.offset = self.MatchBlockRadius, self.m_ws, self.m_offset
            cfg.origin_width = data.m_OriginSize[0] or W
            cfg.image = [cams[0].image, cams[1].image]
            cfg.mask = [cams[0].mask, cams[1].mask]
            cfg.Q, cfg.R_final, cfg.T_final = self.Q, self.R_final, self.T_final
            cfg.verbose = self.Verbose
            res = self._ctx.match_pair(cfg)
            self.margin = [res.margin[0], res.margin[1]]
            cams[0].bound = res.margin[0]     # .cpp:27-28
            cams[1].bound = res.margin[1]
            self.disparity = res.disparity
            if self.Verbose >= 1:
                print("\tconverting disparity to cloud %d..." % CamPair)
            if getattr(data, "isoutput", 0):   # .cpp:707-730,753-757: cloud%d.ply in the working directory
                write_ply("cloud%d.ply" % CamPair, res.xyz, res.bgr)
            sink = self.m_CloudOptimization
            if sink is not None:
                if hasattr(sink, "InsertPoints"):
                    sink.InsertPoints(res.xyz, res.bgr)
                else:
                    for p in res.xyz:
                        sink.InsertPoint(p)
                if hasattr(sink, "filter"):
                    sink.filter(CamPair)      # .cpp:31
            self.last_result = res


class CloudOptimization:
    """The part of CCloudOptimization (CloudOptimization/CCloudOptimization.cpp) that sits on the stereo path:
    Init (:40-57: only the per-pair filter's parameters are used), InsertPoint (:59-62), filter(idx) (:64-147: the
    StatisticalOutlierRemoval + NormalEstimation + normal flip of :82-121 on the GPU, with `use_outrem` the RadiusOutlierRemoval of
    :90-96 between them, which the shipped reference has commented out; the mesh / texture tooling
    after :123 is Windows executables and out of scope), run() (:348-389: MLS over the merged cloud + the normal flip
    on the GPU), mesh() (where run() calls the external Poisson mesher after :389: the dense-grid Poisson surface and trim on the GPU),
    trim_mesh() (mesh.bat's SurfaceTrimmer: the surface cut where the samples' density falls below a depth, on the GPU),
    clean_mesh() (what meshlab.bat goes on to do: Laplacian smoothing and the removal of isolated pieces and bad faces, on the GPU),
    close_mesh_holes() (its last filter: small border loops filled with their least-area triangulation, on the GPU),
    decimate_mesh() (decimation.mlx: the mesh thinned to a face count by quadric edge collapses, on the GPU),
    subdivide_mesh() (subdiv.mlx: the mesh refined by Loop subdivision, Loop's own weights, on the GPU),
    color_mesh() (where run() ends with TextureStitcher: the mesh's vertices coloured from every camera's rectified image, on the
    GPU), stitch_mesh() (the tool's seam removal: the views' exposure seams levelled in those colours, on the GPU), fill_mesh_colors() (the vertices no view saw filled from the colours around them, on the GPU).  `cloud_normals` accumulates what the
    reference's global `*cloud_normals += *cloud_normal` (:123) does: per pair (xyz float32 [m,3], normals float32 [m,4])."""

    def __init__(self, ctx: Context | None = None, device: int = 0):
        self._ctx = ctx or Context(device)
        self._pts = []
        self._bgr = None
        self.cloud_normals = []
        self.cloud_bgr = []      # colours of the surviving points, per pair (imagePyrm[top][0], .cpp:756)
        self.stats = []
        self.use_outrem = False  # the RadiusOutlierRemoval of :90-96, commented out in the shipped reference: True runs it with Init's two values

    def Init(self, sor_meank, sor_stdThres, outrem_neighbor, outrem_radius, mls_radius, ImageData, isdelete_=False):
        self.m_sor_meank, self.m_sor_stdThres, self.m_mls_radius = sor_meank, sor_stdThres, mls_radius
        self.m_outrem_neighbor, self.m_outrem_radius = outrem_neighbor, outrem_radius   # :43-44
        self.isdelete = bool(isdelete_)
        self.m_ImageData = ImageData
        self.CamCenter = [np.asarray(c[0].CamCenter if c[0].CamCenter is not None else np.zeros(3), np.float32).ravel()
                          for c in ImageData.cam]

    def InsertPoint(self, p):
        self._pts.append(np.asarray(p, np.float64).ravel()[:3])

    def InsertPoints(self, xyz, bgr=None):
        self._pts = [np.asarray(xyz, np.float64).reshape(-1, 3)]
        self._bgr = None if bgr is None else np.asarray(bgr, np.uint8).reshape(-1, 3)

    def filter(self, idx):
        xyz = (np.concatenate([np.atleast_2d(p) for p in self._pts]) if self._pts else np.zeros((0, 3))).astype(np.float32)
        if self.use_outrem:   # (set on every call, on or off: the setting is the context's, and other users of it may have changed it)
            self._ctx.set_filter_outrem(self.m_outrem_neighbor, self.m_outrem_radius)
        else:
            self._ctx.set_filter_outrem(None, None)
        kept, nrm, st = self._ctx.filter_cloud(xyz, self.m_sor_meank, self.m_sor_stdThres, self.m_mls_radius, self.CamCenter[idx])
        st["outrem"] = self._ctx.filter_last_outrem()
        self.cloud_normals.append((xyz[kept], nrm))
        self.cloud_bgr.append(self._bgr[kept] if self._bgr is not None and len(self._bgr) == len(xyz)
                              else np.zeros((len(kept), 3), np.uint8))
        self.stats.append(st)
        self._pts = []   # cloud_in->clear(), :145
        self._bgr = None

    def run(self):
        """The MLS block of CCloudOptimization::run (:348-389): the pairs' filtered clouds concatenated in pair order (copyPointCloud,
        :353), MovingLeastSquares with m_mls_radius, polynomial order 1 and normals (:355-364), each normal negated where it disagrees
        with its input point's filter normal (:378-385).  With isdelete (Init's isdelete_) the multi-view duplicate deletion
        (:152-346) runs first on the GPU and the MLS reads cloud_normals[indicesptr] (:352); self.indicesptr and self.dedup_stats
        keep what it did.  Stores and returns cloud_ms_normals = (xyz float32 [m,3], normals float32 [m,4], src_index int32 [m] into
        the merged cloud: indicesptr[idx_in_orig] with isdelete); write_ply_pointnormal writes it as savePLYFileBinary does (:389)."""
        if self.cloud_normals:
            xyz = np.concatenate([c[0] for c in self.cloud_normals]).astype(np.float32)
            ref = np.concatenate([c[1] for c in self.cloud_normals]).astype(np.float32)
        else:
            xyz, ref = np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32)
        if getattr(self, "isdelete", False):
            cams = self.m_ImageData.cam
            if any(c.P is None or c.image is None or c.mask is None for pair in cams for c in pair[:2]) or \
                    any(pair[0].bound is None or pair[0].CamCenter is None for pair in cams):
                raise ValueError("CloudOptimization.run: isdelete = true (the multi-view duplicate deletion, CCloudOptimization.cpp:152-346) "
                                 "needs every camera's P, image and mask and the left views' bound and CamCenter, as Rectify and "
                                 "MatchAllLayer leave them; pre-rectified input carries no P")
            self.indicesptr, self.dedup_stats = self._ctx.dedup_cloud(xyz, ref, cams)
            ox, on, oi = self._ctx.mls_cloud(xyz[self.indicesptr], self.m_mls_radius, 1, ref[self.indicesptr])
            self.cloud_ms_normals = (ox, on, self.indicesptr[oi])
        else:
            self.cloud_ms_normals = self._ctx.mls_cloud(xyz, self.m_mls_radius, 1, ref)
        return self.cloud_ms_normals

    def mesh(self, depth=9, scale=1.1, trim_cells=4, rel_residual=POISSON_REL_RESIDUAL, max_cycles=POISSON_MAX_CYCLES, samples_per_node=None,
             kernel_depth=0, band_bricks=None, band_max_iterations=POISSON_BAND_MAX_ITERATIONS, band_samples_per_node=None):
        """Where CCloudOptimization::run hands bigcloud.ply to the Poisson mesher (after :389): the surface of cloud_ms_normals, run()'s
        result, by the dense-grid Poisson reconstruction and trim on the GPU (Context.poisson_mesh).  run() keeps its result on the
        host, so the host entry point is used.  samples_per_node (mesh.bat: 2, script1.mlx: 3) selects the density-adaptive splat
        (Context.poisson_mesh_weighted; kernel_depth as there); None is the plain call.  band_bricks (1..4) selects the banded call
        (Context.poisson_mesh_banded; script1.mlx's OctDepth 10): depth is then the finest depth, 6..10, and trim_cells at most
        8 band_bricks - 1; it does not combine with samples_per_node (ValueError).  The density-adaptive splat on the band has a switch of its
        own because that refusal stays as it is: band_samples_per_node (script1.mlx: 3) with band_bricks selects
        Context.poisson_mesh_banded_weighted, with kernel_depth (0 or 3..depth - 1) passed through; without band_bricks it is a ValueError.
        Stores and returns (vertices float32 [nv,3], faces int32 [nf,3], stats)."""
        if getattr(self, "cloud_ms_normals", None) is None:
            raise ValueError("CloudOptimization.mesh: run() first (it meshes run()'s smoothed, oriented cloud)")
        if band_bricks is not None and samples_per_node is not None:
            raise ValueError("CloudOptimization.mesh: band_bricks and samples_per_node do not combine (the density-adaptive splat is not built on the band)")
        if band_samples_per_node is not None and band_bricks is None:
            raise ValueError("CloudOptimization.mesh: band_samples_per_node needs band_bricks (without the band, samples_per_node selects the density-adaptive splat)")
        xyz, nrm = self.cloud_ms_normals[0], self.cloud_ms_normals[1]
        if band_bricks is not None and band_samples_per_node is not None:
            self.mesh_result = self._ctx.poisson_mesh_banded_weighted(xyz, nrm, depth, scale, trim_cells, rel_residual, max_cycles, band_bricks, band_max_iterations,
                                                                      band_samples_per_node, kernel_depth)
        elif band_bricks is not None:
            self.mesh_result = self._ctx.poisson_mesh_banded(xyz, nrm, depth, scale, trim_cells, rel_residual, max_cycles, band_bricks, band_max_iterations)
        elif samples_per_node is None:
            self.mesh_result = self._ctx.poisson_mesh(xyz, nrm, depth, scale, trim_cells, rel_residual, max_cycles)
        else:
            self.mesh_result = self._ctx.poisson_mesh_weighted(xyz, nrm, depth, scale, trim_cells, rel_residual, max_cycles, samples_per_node, kernel_depth)
        self.mesh_grid_step = self.mesh_result[2]["h"]
        self._mesh_box = (depth, scale)
        self.mesh_colors = None
        return self.mesh_result

    def trim_mesh(self, kernel_depth=0, samples_per_node=2.0, smooth_steps=100, trim=7.0, island_ratio=0.01):
        """Where mesh.bat follows PoissonRecon --density with SurfaceTrimmer --smooth 100 --trim 7 --aRatio 0.01: the density trim of
        mesh_result (Context.mesh_trim_last on the mesh mesh() left with the context) with the samples and the depth / scale mesh() used;
        call mesh(trim_cells=0) so that the occupancy trim has not cut the surface already.  Replaces mesh_result."""
        if getattr(self, "mesh_result", None) is None:
            raise ValueError("CloudOptimization.trim_mesh: mesh() first (it trims mesh()'s surface by the density of mesh()'s samples)")
        depth, scale = self._mesh_box
        self.mesh_result = self._ctx.mesh_trim_last(self.cloud_ms_normals[0], self.cloud_ms_normals[1], depth, scale, kernel_depth, samples_per_node,
                                                    smooth_steps, trim, island_ratio)
        self.mesh_colors = None
        return self.mesh_result

    def clean_mesh(self, smooth_steps=5, cotangent=True, boundary=True, min_piece=0.10, relative=True, duplicates=True, zero_area=True,
                   nonmanifold=True):
        """Where meshlab.bat goes on after its Poisson filter (script1.mlx's Laplacian Smooth, script2.mlx's clean-up -> bigmesh.ply):
        Context.mesh_clean_last on the mesh mesh() left with the context, without a host round trip.  Replaces mesh_result."""
        if getattr(self, "mesh_result", None) is None:
            raise ValueError("CloudOptimization.clean_mesh: mesh() first (it smooths and cleans mesh()'s surface)")
        self.mesh_result = self._ctx.mesh_clean_last(smooth_steps, cotangent, boundary, min_piece, relative, duplicates, zero_area, nonmanifold)
        self.mesh_colors = None
        return self.mesh_result

    def close_mesh_holes(self, max_hole_size=30):
        """Where meshlab.bat's script2.mlx ends with "Close Holes" (MaxHoleSize 30): every simple border loop of mesh_result of at most
        max_hole_size edges filled with its least-area triangulation (Context.mesh_close_holes_last on the mesh mesh() / trim_mesh() /
        clean_mesh() left with the context, without a host round trip).  Replaces mesh_result."""
        if getattr(self, "mesh_result", None) is None:
            raise ValueError("CloudOptimization.close_mesh_holes: mesh() first (it closes the small holes of mesh()'s surface)")
        self.mesh_result = self._ctx.mesh_close_holes_last(max_hole_size)
        self.mesh_colors = None
        return self.mesh_result

    def decimate_mesh(self, target_faces=100000, **params):
        """Where a user of the reference reaches for Demo/meshlab/decimation.mlx ("Quadric Edge Collapse Decimation", TargetFaceNum 100000):
        mesh_result thinned to target_faces faces by rounds of independent edge collapses (Context.mesh_decimate_last on the mesh mesh() /
        clean_mesh() / close_mesh_holes() left with the context, without a host round trip).  params: the script's other
        parameters, Context.mesh_decimate_params'.  Replaces mesh_result."""
        if getattr(self, "mesh_result", None) is None:
            raise ValueError("CloudOptimization.decimate_mesh: mesh() first (it decimates mesh()'s surface)")
        self.mesh_result = self._ctx.mesh_decimate_last(target_faces=target_faces, **params)
        self.mesh_colors = None
        return self.mesh_result

    def subdivide_mesh(self, iterations=3, threshold_fraction=0.01, **params):
        """Where a user of the reference reaches for Demo/meshlab/subdiv.mlx ("Subdivision Surfaces: Loop", Iterations 3, Threshold 1 % of
        the box diagonal): mesh_result refined by Loop subdivision of every edge longer than the threshold (Context.mesh_subdivide_last on
        the mesh mesh() / clean_mesh() / decimate_mesh() left with the context, without a host round trip) -- call it
        before color_mesh(), whose colour resolution is the vertex density.  Loop's own weights only (the script's LoopWeight 2 is not
        built); positions only: colours computed before are dropped.  params: Context.mesh_subdivide_params' (threshold: an absolute
        length, read when threshold_fraction is 0).  Replaces mesh_result."""
        if getattr(self, "mesh_result", None) is None:
            raise ValueError("CloudOptimization.subdivide_mesh: mesh() first (it subdivides mesh()'s surface)")
        self.mesh_result = self._ctx.mesh_subdivide_last(iterations=iterations, threshold_fraction=threshold_fraction, **params)
        self.mesh_colors = None
        return self.mesh_result

    def color_mesh(self, mode=1, min_cos=0.2, depth_eps=None):
        """Where CCloudOptimization::run calls TextureStitcher on bigmesh.ply (:394-397): the colours of mesh_result's vertices from every
        camera's rectified image (Context.mesh_color_last on the mesh mesh() / clean_mesh() left with the context; the mesh itself is
        untouched).  depth_eps defaults to twice the Poisson grid step.  Stores and returns
        mesh_colors = (rgb uint8 [nv,3], best_view int32 [nv], stats)."""
        if getattr(self, "mesh_result", None) is None:
            raise ValueError("CloudOptimization.color_mesh: mesh() first (it colours mesh()'s surface)")
        cams = self.m_ImageData.cam
        if any(c.P is None or c.image is None for pair in cams for c in pair[:2]):
            raise ValueError("CloudOptimization.color_mesh: the mesh colouring (where CCloudOptimization::run calls TextureStitcher, "
                             "CCloudOptimization.cpp:394-397) needs every camera's P and image, as Rectify leaves them; pre-rectified input "
                             "carries no P")
        if depth_eps is None:
            depth_eps = 2.0 * self.mesh_grid_step
        self.mesh_colors = self._ctx.mesh_color_last(cams, depth_eps, mode, min_cos)
        return self.mesh_colors

    def stitch_mesh(self, min_cos=0.2, depth_eps=None, lam=0.01, iterations=0, reduction=1e-4, seam_gradient=True):
        """The other half of TextureStitcher's job (:394-397): mesh_result's vertices coloured by their best view, then the views'
        exposure seams levelled by the screened gradient-domain solve of DESIGN.md 9 f10 (Context.mesh_stitch_last; the mesh itself is
        untouched).  depth_eps defaults to twice the Poisson grid step.  Stores and returns
        mesh_colors = (rgb uint8 [nv,3], best_view int32 [nv], stats)."""
        if getattr(self, "mesh_result", None) is None:
            raise ValueError("CloudOptimization.stitch_mesh: mesh() first (it colours mesh()'s surface)")
        cams = self.m_ImageData.cam
        if any(c.P is None or c.image is None for pair in cams for c in pair[:2]):
            raise ValueError("CloudOptimization.stitch_mesh: the mesh colouring (where CCloudOptimization::run calls TextureStitcher, "
                             "CCloudOptimization.cpp:394-397) needs every camera's P and image, as Rectify leaves them; pre-rectified input "
                             "carries no P")
        if depth_eps is None:
            depth_eps = 2.0 * self.mesh_grid_step
        self.mesh_colors = self._ctx.mesh_stitch_last(cams, depth_eps, min_cos, lam, iterations, reduction, seam_gradient)
        return self.mesh_colors

    def fill_mesh_colors(self, max_rounds=0, iterations=0, reduction=1e-4):
        """After color_mesh() or stitch_mesh(): TextureStitcher hands back a mesh that is coloured everywhere, so every vertex no view saw
        ((127, 127, 127), best_view -1) that is connected to a coloured one takes the harmonic extension of the colours around it on the
        mesh graph (Context.mesh_fill_colors_last on the colours left with the context).  max_rounds > 0 fills only the
        vertices within that many edges of a coloured one.  Coloured vertices keep their bytes and best_view is unchanged: a filled
        vertex keeps -1.  Stores and returns mesh_colors = (rgb uint8 [nv,3], best_view int32 [nv], stats)."""
        if getattr(self, "mesh_colors", None) is None:
            raise ValueError("CloudOptimization.fill_mesh_colors: color_mesh() or stitch_mesh() first (it fills their uncoloured vertices)")
        self.mesh_colors = self._ctx.mesh_fill_colors_last(max_rounds, iterations, reduction)
        return self.mesh_colors
