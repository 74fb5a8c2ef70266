"""The surface stages (csrc/rsm_poisson.hip, csrc/rsm_mesh.hip): dense-grid Poisson surface and trim, smoothing and clean-up, the closing of small holes, the
decimation, colours from the rig's views and the levelling of their seams."""
import ctypes as C

import numpy as np

from . import _lib
from ._context import ContextBase, _normals4, _p, _u8, _views
from ._lib import MeshCleanParams, MeshCloseParams, MeshColorParams, MeshDecimateParams, MeshFillParams, MeshStitchParams, MeshSubdivideParams, MeshTrimParams, PoissonBandParams, PoissonDensityParams, PoissonParams

# the solve's default stopping residual: one decade above the 4.2e-6 the float32 solver reaches at depth 9
POISSON_REL_RESIDUAL = 4e-5
POISSON_MAX_CYCLES = 100
# the band solve's iteration cap: four times the 41 to 50 iterations the sphere fixtures take to POISSON_REL_RESIDUAL
POISSON_BAND_MAX_ITERATIONS = 200
# meshlab.bat's script1 / script2 settings: the defaults of mesh_clean, mesh_clean_device and mesh_clean_last
_MC = dict(smooth_steps=5, cotangent=True, boundary=True, min_piece=0.10, relative=True, duplicates=True, zero_area=True, nonmanifold=True)
# mesh.bat's PoissonRecon --samplesPerNode 2 and SurfaceTrimmer --smooth 100 --trim 7 --aRatio 0.01: the defaults of mesh_trim, mesh_trim_device and mesh_trim_last
_MT = dict(kernel_depth=0, samples_per_node=2.0, smooth_steps=100, trim=7.0, island_ratio=0.01)


def _mesh_arrays(vertices, faces):
    return np.ascontiguousarray(vertices, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)


class MeshPart(ContextBase):
    # ---- surface from the oriented cloud: dense-grid Poisson + trim (csrc/k_poisson.hip) ----
    def poisson_last_mesh(self, n_vertices, n_faces):
        """The context's last mesh on the host: (vertices float32 [nv,3], faces int32 [nf,3])."""
        v = np.zeros((max(n_vertices, 1), 3), np.float32)
        f = np.zeros((max(n_faces, 1), 3), np.int32)
        self._chk(self._lib.rsm_poisson_last_mesh(self._h, _p(v), _p(f)))
        return v[:n_vertices].copy(), f[:n_faces].copy()

    def _poisson(self, fn, xyz, nrm, n, depth, scale, trim_cells, rel_residual, max_cycles):
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.POISSON_STATS)()
        prm = PoissonParams(int(depth), float(scale), float(rel_residual), int(max_cycles), int(trim_cells))
        status = fn(self._h, xyz, nrm, n, C.byref(prm), C.byref(nv), C.byref(nf), st)
        if status < 0:
            self._chk(status)
        stats = dict(n_valid=int(st[0]), n_invalid=int(st[1]), residual=float(st[2]), cycles=int(st[3]), iso=float(st[4]),
                     origin=(float(st[5]), float(st[6]), float(st[7])), h=float(st[8]), N=int(st[9]), n_vertices_untrimmed=int(st[10]),
                     n_faces_untrimmed=int(st[11]), status=int(status), converged=status == 0)
        return int(nv.value), int(nf.value), stats

    def poisson_mesh(self, xyz, normals, depth=9, scale=1.1, trim_cells=4, rel_residual=POISSON_REL_RESIDUAL, max_cycles=POISSON_MAX_CYCLES):
        """Unscreened Poisson reconstruction on a dense 2^depth grid, marching tetrahedra and the occupancy trim, of a host cloud:
        xyz [n,3] float32 with normals [n,4] or [n,3] (what mls_cloud returns).  Returns (vertices float32 [nv,3], faces int32 [nf,3],
        stats dict); stats['converged'] is False (status 1) when max_cycles came before rel_residual -- the mesh is that of the
        chi reached.  Samples that are not finite or have a zero normal take no part (stats['n_invalid'])."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = _normals4(normals, len(xyz))
        nv, nf, stats = self._poisson(self._lib.rsm_poisson_mesh, _p(xyz), _p(nrm), len(xyz), depth, scale, trim_cells, rel_residual, max_cycles)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def poisson_mesh_device(self, xyz_ptr, normals_ptr, n, depth=9, scale=1.1, trim_cells=4, rel_residual=POISSON_REL_RESIDUAL,
                            max_cycles=POISSON_MAX_CYCLES):
        """rsm_poisson_mesh_device on device buffers (addresses): n float xyz (stride 3) and n float4 normals, as mls_cloud_device leaves
        them.  The mesh stays with the context: returns (n_vertices, n_faces, stats); poisson_last_mesh[_device] copies it out."""
        return self._poisson(self._lib.rsm_poisson_mesh_device, xyz_ptr, normals_ptr, n, depth, scale, trim_cells, rel_residual, max_cycles)

    def poisson_last_mesh_device(self, vertices_ptr, faces_ptr):
        """Copies the context's last mesh into caller-owned device buffers (addresses; either may be 0)."""
        self._chk(self._lib.rsm_poisson_last_mesh_device(self._h, vertices_ptr, faces_ptr))

    def poisson_rhs(self, xyz, normals, depth, scale=1.1):
        """Stage: samples -> (grid (ox, oy, oz, h), b float64 [N,N,N] indexed [k,j,i], occ uint8 [N,N,N], (valid, invalid))."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        nrm = _normals4(normals, n)
        N = 1 << int(depth)
        grid = np.zeros(4, np.float64)
        b = np.zeros((N, N, N), np.float64)
        occ = np.zeros((N, N, N), np.uint8)
        counts = np.zeros(2, np.int64)
        prm = PoissonParams(int(depth), float(scale), 0.5, 1, 0)
        self._chk(self._lib.rsm_stage_poisson_rhs(self._h, _p(xyz), _p(nrm), n, C.byref(prm), _p(grid), _p(b), _p(occ), _p(counts)))
        return grid, b, occ, (int(counts[0]), int(counts[1]))

    # ---- the density-adaptive form: PoissonRecon's --samplesPerNode (csrc/k_poisson_density.hip) ----
    def _poisson_weighted(self, fn, xyz, nrm, n, depth, scale, trim_cells, rel_residual, max_cycles, samples_per_node, kernel_depth):
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.POISSON_WEIGHTED_STATS)()
        prm = PoissonParams(int(depth), float(scale), float(rel_residual), int(max_cycles), int(trim_cells))
        dpr = PoissonDensityParams(int(kernel_depth), float(samples_per_node))
        status = fn(self._h, xyz, nrm, n, C.byref(prm), C.byref(dpr), C.byref(nv), C.byref(nf), st)
        if status < 0:
            self._chk(status)
        stats = dict(n_valid=int(st[0]), n_invalid=int(st[1]), residual=float(st[2]), cycles=int(st[3]), iso=float(st[4]),
                     origin=(float(st[5]), float(st[6]), float(st[7])), h=float(st[8]), N=int(st[9]), n_vertices_untrimmed=int(st[10]),
                     n_faces_untrimmed=int(st[11]), kernel_depth=int(st[12]), min_sample_depth=float(st[13]), n_below_depth=int(st[14]),
                     weight_sum=float(st[15]), status=int(status), converged=status == 0)
        return int(nv.value), int(nf.value), stats

    def poisson_mesh_weighted(self, xyz, normals, depth=9, scale=1.1, trim_cells=4, rel_residual=POISSON_REL_RESIDUAL, max_cycles=POISSON_MAX_CYCLES,
                              samples_per_node=2.0, kernel_depth=0):
        """poisson_mesh with the density-adaptive splat, what PoissonRecon's --samplesPerNode does (mesh.bat: 2, script1.mlx: 3): every
        sample is spread at the grid levels around the depth at which a node would hold samples_per_node of the samples near it (their
        density from a count splat on 2^kernel_depth nodes per axis; 0 = depth - 2) and weighs the inverse of that density, so that
        thinly sampled parts of the surface hold their place.  Returns (vertices, faces, stats dict); beyond poisson_mesh's keys the
        stats hold kernel_depth, min_sample_depth, n_below_depth (samples spread below the finest level) and weight_sum."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = _normals4(normals, len(xyz))
        nv, nf, stats = self._poisson_weighted(self._lib.rsm_poisson_mesh_weighted, _p(xyz), _p(nrm), len(xyz), depth, scale, trim_cells, rel_residual,
                                               max_cycles, samples_per_node, kernel_depth)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def poisson_mesh_weighted_device(self, xyz_ptr, normals_ptr, n, depth=9, scale=1.1, trim_cells=4, rel_residual=POISSON_REL_RESIDUAL,
                                     max_cycles=POISSON_MAX_CYCLES, samples_per_node=2.0, kernel_depth=0):
        """rsm_poisson_mesh_weighted_device on device buffers (addresses), as poisson_mesh_device: (n_vertices, n_faces, stats)."""
        return self._poisson_weighted(self._lib.rsm_poisson_mesh_weighted_device, xyz_ptr, normals_ptr, n, depth, scale, trim_cells, rel_residual, max_cycles,
                                      samples_per_node, kernel_depth)

    def poisson_rhs_weighted(self, xyz, normals, depth, scale=1.1, samples_per_node=2.0, kernel_depth=0, depth_in=None):
        """Stage: samples -> (grid (ox, oy, oz, h), b float64 [N,N,N] indexed [k,j,i], occ uint8 [N,N,N], (valid, invalid), rho float64 [n],
        w float64 [n], d float64 [n]) of the density-adaptive splat; depth_in (float64 [n]): every sample's depth from the caller."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        nrm = _normals4(normals, n)
        N = 1 << int(depth)
        grid = np.zeros(4, np.float64)
        b = np.zeros((N, N, N), np.float64)
        occ = np.zeros((N, N, N), np.uint8)
        counts = np.zeros(2, np.int64)
        rho, w, d = (np.zeros(max(n, 1), np.float64) for _ in range(3))
        din = None if depth_in is None else np.ascontiguousarray(depth_in, np.float64).reshape(-1)
        assert din is None or len(din) == n
        prm = PoissonParams(int(depth), float(scale), 0.5, 1, 0)
        dpr = PoissonDensityParams(int(kernel_depth), float(samples_per_node))
        self._chk(self._lib.rsm_stage_poisson_rhs_weighted(self._h, _p(xyz), _p(nrm), n, C.byref(prm), C.byref(dpr), None if din is None else _p(din), _p(grid),
                                                           _p(b), _p(occ), _p(counts), _p(rho), _p(w), _p(d)))
        return grid, b, occ, (int(counts[0]), int(counts[1])), rho[:n].copy(), w[:n].copy(), d[:n].copy()

    # ---- one level finer on a band of bricks: script1.mlx's OctDepth 10 (csrc/k_poisson_band.hip) ----
    def _poisson_banded(self, fn, xyz, nrm, n, depth, scale, trim_cells, rel_residual, max_cycles, band_bricks, max_iterations):
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.POISSON_BAND_STATS)()
        prm = PoissonParams(int(depth), float(scale), float(rel_residual), int(max_cycles), int(trim_cells))
        bpr = PoissonBandParams(int(band_bricks), int(max_iterations))
        status = fn(self._h, xyz, nrm, n, C.byref(prm), C.byref(bpr), C.byref(nv), C.byref(nf), st)
        if status < 0:
            self._chk(status)
        stats = dict(n_valid=int(st[0]), n_invalid=int(st[1]), residual=float(st[2]), iterations=int(st[3]), iso=float(st[4]),
                     origin=(float(st[5]), float(st[6]), float(st[7])), h=float(st[8]), N=int(st[9]), n_vertices_untrimmed=int(st[10]),
                     n_faces_untrimmed=int(st[11]), active_bricks=int(st[12]), occupied_bricks=int(st[13]), coarse_cycles=int(st[14]),
                     coarse_residual=float(st[15]), residual_before=float(st[16]), status=int(status), converged=status == 0)
        return int(nv.value), int(nf.value), stats

    def poisson_mesh_banded(self, xyz, normals, depth=10, scale=1.1, trim_cells=7, rel_residual=POISSON_REL_RESIDUAL, max_cycles=POISSON_MAX_CYCLES,
                            band_bricks=1, max_iterations=POISSON_BAND_MAX_ITERATIONS):
        """poisson_mesh one level finer than the dense grid reaches: depth (6..10) is the FINEST depth; the dense solve runs at depth - 1 and
        the level of 2^depth nodes per axis exists only on the bricks (8^3 nodes) within band_bricks (1..4) of a brick that holds a sample,
        where the field is corrected by at most max_iterations conjugate-gradient iterations.  trim_cells <= 8 band_bricks - 1 (script1.mlx
        at depth 10 corresponds to trim_cells 8, which needs band_bricks 2); with trim_cells = 0 the mesh has borders where the band ends.
        Returns (vertices, faces, stats dict); beyond poisson_mesh's keys (iterations for cycles) the stats hold active_bricks,
        occupied_bricks, coarse_cycles, coarse_residual and residual_before (the band residual of the prolonged coarse field)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = _normals4(normals, len(xyz))
        nv, nf, stats = self._poisson_banded(self._lib.rsm_poisson_mesh_banded, _p(xyz), _p(nrm), len(xyz), depth, scale, trim_cells, rel_residual, max_cycles,
                                             band_bricks, max_iterations)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def poisson_mesh_banded_device(self, xyz_ptr, normals_ptr, n, depth=10, scale=1.1, trim_cells=7, rel_residual=POISSON_REL_RESIDUAL,
                                   max_cycles=POISSON_MAX_CYCLES, band_bricks=1, max_iterations=POISSON_BAND_MAX_ITERATIONS):
        """rsm_poisson_mesh_banded_device on device buffers (addresses), as poisson_mesh_device: (n_vertices, n_faces, stats)."""
        return self._poisson_banded(self._lib.rsm_poisson_mesh_banded_device, xyz_ptr, normals_ptr, n, depth, scale, trim_cells, rel_residual, max_cycles,
                                    band_bricks, max_iterations)

    def poisson_band_rhs(self, xyz, normals, depth, scale=1.1, band_bricks=1, chi_c=None, max_bricks=0, rel_residual=POISSON_REL_RESIDUAL,
                         max_cycles=POISSON_MAX_CYCLES):
        """Stage: samples -> dict grid (ox, oy, oz, h of the fine grid), bricks int32 [S] (ascending linear brick indices), b float64 [S,512],
        occ uint8 [S,512], g float32 [S,512] (brick-major: element lx + 8 (ly + 8 lz)), counts (valid, invalid, active, occupied), status.
        chi_c (float32 [N/2]^3 indexed [k,j,i]): the coarse field the guess is prolonged from; None: the dense solve at depth - 1."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        nrm = _normals4(normals, n)
        room = ((1 << int(depth)) >> 3) ** 3 if 6 <= int(depth) <= 10 else 1
        room = min(room, _lib.POISSON_BAND_MAX_BRICKS if not max_bricks else int(max_bricks))
        grid = np.zeros(4, np.float64)
        bricks = np.zeros(max(room, 1), np.int32)
        b = np.zeros((max(room, 1), 512), np.float64)
        occ = np.zeros((max(room, 1), 512), np.uint8)
        g = np.zeros((max(room, 1), 512), np.float32)
        counts = np.zeros(4, np.int64)
        cc = None if chi_c is None else np.ascontiguousarray(chi_c, np.float32)
        assert cc is None or cc.shape == ((1 << int(depth)) >> 1,) * 3
        prm = PoissonParams(int(depth), float(scale), float(rel_residual), int(max_cycles), 0)
        bpr = PoissonBandParams(int(band_bricks), 1)
        status = self._lib.rsm_stage_poisson_band_rhs(self._h, _p(xyz), _p(nrm), n, C.byref(prm), C.byref(bpr), None if cc is None else _p(cc), int(max_bricks),
                                                      room, _p(grid), _p(bricks), _p(b), _p(occ), _p(g), _p(counts))
        if status < 0:
            self._chk(status)
        S = int(counts[2])
        return dict(grid=grid, bricks=bricks[:S].copy(), b=b[:S].copy(), occ=occ[:S].copy(), g=g[:S].copy(), counts=tuple(int(v) for v in counts), status=int(status))

    # ---- the banded call with the density-adaptive splat: script1.mlx's OctDepth 10 and SamplesPerNode 3 (csrc/k_poisson_band_density.hip) ----
    def _poisson_banded_weighted(self, fn, xyz, nrm, n, depth, scale, trim_cells, rel_residual, max_cycles, band_bricks, max_iterations, samples_per_node, kernel_depth):
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.POISSON_BAND_WEIGHTED_STATS)()
        prm = PoissonParams(int(depth), float(scale), float(rel_residual), int(max_cycles), int(trim_cells))
        bpr = PoissonBandParams(int(band_bricks), int(max_iterations))
        dpr = PoissonDensityParams(int(kernel_depth), float(samples_per_node))
        status = fn(self._h, xyz, nrm, n, C.byref(prm), C.byref(bpr), C.byref(dpr), C.byref(nv), C.byref(nf), st)
        if status < 0:
            self._chk(status)
        stats = dict(n_valid=int(st[0]), n_invalid=int(st[1]), residual=float(st[2]), iterations=int(st[3]), iso=float(st[4]),
                     origin=(float(st[5]), float(st[6]), float(st[7])), h=float(st[8]), N=int(st[9]), n_vertices_untrimmed=int(st[10]),
                     n_faces_untrimmed=int(st[11]), active_bricks=int(st[12]), occupied_bricks=int(st[13]), coarse_cycles=int(st[14]),
                     coarse_residual=float(st[15]), residual_before=float(st[16]), kernel_depth=int(st[17]), min_sample_depth=float(st[18]),
                     n_below_depth=int(st[19]), sum_w=float(st[20]), status=int(status), converged=status == 0)
        return int(nv.value), int(nf.value), stats

    def poisson_mesh_banded_weighted(self, xyz, normals, depth=10, scale=1.1, trim_cells=7, rel_residual=POISSON_REL_RESIDUAL, max_cycles=POISSON_MAX_CYCLES,
                                     band_bricks=1, max_iterations=POISSON_BAND_MAX_ITERATIONS, samples_per_node=3.0, kernel_depth=0):
        """poisson_mesh_banded with poisson_mesh_weighted's density-adaptive splat (script1.mlx: OctDepth 10 with SamplesPerNode 3): every
        sample's density, weight and depth are the weighted call's at the finest depth; the levels below the finest are dense and reach the
        band through their trilinear prolongation, the finest lives on the bricks, and the dense solve at depth - 1 is the weighted one.
        kernel_depth is 0 (depth - 2) or 3..depth - 1.  Returns (vertices, faces, stats dict): poisson_mesh_banded's keys and kernel_depth,
        min_sample_depth, n_below_depth (samples spread below the finest level) and sum_w."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nrm = _normals4(normals, len(xyz))
        nv, nf, stats = self._poisson_banded_weighted(self._lib.rsm_poisson_mesh_banded_weighted, _p(xyz), _p(nrm), len(xyz), depth, scale, trim_cells, rel_residual,
                                                      max_cycles, band_bricks, max_iterations, samples_per_node, kernel_depth)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def poisson_mesh_banded_weighted_device(self, xyz_ptr, normals_ptr, n, depth=10, scale=1.1, trim_cells=7, rel_residual=POISSON_REL_RESIDUAL,
                                            max_cycles=POISSON_MAX_CYCLES, band_bricks=1, max_iterations=POISSON_BAND_MAX_ITERATIONS, samples_per_node=3.0,
                                            kernel_depth=0):
        """rsm_poisson_mesh_banded_weighted_device on device buffers (addresses), as poisson_mesh_device: (n_vertices, n_faces, stats)."""
        return self._poisson_banded_weighted(self._lib.rsm_poisson_mesh_banded_weighted_device, xyz_ptr, normals_ptr, n, depth, scale, trim_cells, rel_residual,
                                             max_cycles, band_bricks, max_iterations, samples_per_node, kernel_depth)

    def poisson_band_rhs_weighted(self, xyz, normals, depth, scale=1.1, band_bricks=1, samples_per_node=3.0, kernel_depth=0, depth_in=None, chi_c=None,
                                  max_bricks=0, rel_residual=POISSON_REL_RESIDUAL, max_cycles=POISSON_MAX_CYCLES):
        """Stage: poisson_band_rhs with the density-adaptive splat -> its dict (grid, bricks, b float64 [S,512], occ, g, counts, status) and
        rho, w, d float64 [n].  depth_in (float64 [n]): every sample's depth from the caller.  chi_c None: the weighted dense solve at depth - 1."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        nrm = _normals4(normals, n)
        room = ((1 << int(depth)) >> 3) ** 3 if 6 <= int(depth) <= 10 else 1
        room = min(room, _lib.POISSON_BAND_MAX_BRICKS if not max_bricks else int(max_bricks))
        grid = np.zeros(4, np.float64)
        bricks = np.zeros(max(room, 1), np.int32)
        b = np.zeros((max(room, 1), 512), np.float64)
        occ = np.zeros((max(room, 1), 512), np.uint8)
        g = np.zeros((max(room, 1), 512), np.float32)
        counts = np.zeros(4, np.int64)
        rho, w, d = (np.zeros(max(n, 1), np.float64) for _ in range(3))
        din = None if depth_in is None else np.ascontiguousarray(depth_in, np.float64).reshape(-1)
        assert din is None or len(din) == n
        cc = None if chi_c is None else np.ascontiguousarray(chi_c, np.float32)
        assert cc is None or cc.shape == ((1 << int(depth)) >> 1,) * 3
        prm = PoissonParams(int(depth), float(scale), float(rel_residual), int(max_cycles), 0)
        bpr = PoissonBandParams(int(band_bricks), 1)
        dpr = PoissonDensityParams(int(kernel_depth), float(samples_per_node))
        status = self._lib.rsm_stage_poisson_band_rhs_weighted(self._h, _p(xyz), _p(nrm), n, C.byref(prm), C.byref(bpr), C.byref(dpr), None if din is None else _p(din),
                                                               None if cc is None else _p(cc), int(max_bricks), room, _p(grid), _p(bricks), _p(b), _p(occ), _p(g),
                                                               _p(counts), _p(rho), _p(w), _p(d))
        if status < 0:
            self._chk(status)
        S = int(counts[2])
        return dict(grid=grid, bricks=bricks[:S].copy(), b=b[:S].copy(), occ=occ[:S].copy(), g=g[:S].copy(), counts=tuple(int(v) for v in counts), status=int(status),
                    rho=rho[:n].copy(), w=w[:n].copy(), d=d[:n].copy())

    def poisson_band_solve(self, bricks, depth, b, g, chi_c=None, rel_residual=POISSON_REL_RESIDUAL, max_iterations=POISSON_BAND_MAX_ITERATIONS):
        """Stage: b and g (brick-major [S,512], rounded to float32) on the bricks -> (chi float32 [S,512], residual reached, iterations, status
        0 / 1, residual per iteration, residual before the first).  chi_c (float32 [N/2]^3): gives the guess next to the band; None: 0 there."""
        bricks = np.ascontiguousarray(bricks, np.int32).reshape(-1)
        S = len(bricks)
        b = np.ascontiguousarray(b, np.float32).reshape(S, 512)
        g = np.ascontiguousarray(g, np.float32).reshape(S, 512)
        cc = None if chi_c is None else np.ascontiguousarray(chi_c, np.float32)
        assert cc is None or cc.shape == ((1 << int(depth)) >> 1,) * 3
        chi = np.zeros((max(S, 1), 512), np.float32)
        res, res0, its = C.c_double(), C.c_double(), C.c_int()
        hist = np.zeros(max(1, int(max_iterations)), np.float64)
        status = self._lib.rsm_stage_poisson_band_solve(self._h, _p(bricks), S, int(depth), _p(b), _p(g), None if cc is None else _p(cc), float(rel_residual),
                                                        int(max_iterations), _p(chi), C.byref(res), C.byref(its), C.byref(res0), _p(hist))
        if status < 0:
            self._chk(status)
        return chi[:S].copy(), float(res.value), int(its.value), int(status), hist[:int(its.value)].copy(), float(res0.value)

    def band_iso_mesh(self, bricks, depth, chi, iso, grid, occ=None, trim_cells=0):
        """Stage: a caller's chi (float32 [S,512], brick-major), iso, grid (ox, oy, oz, h) and occ (uint8 [S,512]) -> (vertices, faces)."""
        bricks = np.ascontiguousarray(bricks, np.int32).reshape(-1)
        S = len(bricks)
        chi = np.ascontiguousarray(chi, np.float32).reshape(S, 512)
        grid = np.ascontiguousarray(grid, np.float64).reshape(4)
        o8 = None if occ is None else _u8(occ).reshape(S, 512)
        nv, nf = C.c_int64(), C.c_int64()
        self._chk(self._lib.rsm_stage_band_iso_mesh(self._h, _p(bricks), S, int(depth), _p(chi), float(iso), _p(grid), None if o8 is None else _p(o8),
                                                    int(trim_cells), C.byref(nv), C.byref(nf)))
        return self.poisson_last_mesh(int(nv.value), int(nf.value))

    def poisson_solve(self, b, rel_residual=POISSON_REL_RESIDUAL, max_cycles=POISSON_MAX_CYCLES):
        """Stage: b [N,N,N] (rounded to float32) -> (chi float32 [N,N,N], residual reached, cycles, status 0 / 1, residual per cycle)."""
        b = np.ascontiguousarray(b, np.float32)
        N = b.shape[0]
        depth = int(N).bit_length() - 1
        assert b.shape == (N, N, N) and (1 << depth) == N
        chi = np.zeros_like(b)
        res, cyc = C.c_double(), C.c_int()
        hist = np.zeros(max(1, int(max_cycles)), np.float64)
        status = self._lib.rsm_stage_poisson_solve(self._h, _p(b), depth, float(rel_residual), int(max_cycles), _p(chi), C.byref(res), C.byref(cyc), _p(hist))
        if status < 0:
            self._chk(status)
        return chi, float(res.value), int(cyc.value), int(status), hist[:int(cyc.value)].copy()

    def iso_mesh(self, chi, iso, grid, occ=None, trim_cells=0):
        """Stage: a caller's chi (float32 [N,N,N]), iso, grid (ox, oy, oz, h) and occ -> (vertices, faces)."""
        chi = np.ascontiguousarray(chi, np.float32)
        N = chi.shape[0]
        depth = int(N).bit_length() - 1
        grid = np.ascontiguousarray(grid, np.float64).reshape(4)
        o8 = None if occ is None else _u8(occ)
        nv, nf = C.c_int64(), C.c_int64()
        self._chk(self._lib.rsm_stage_iso_mesh(self._h, _p(chi), depth, float(iso), _p(grid), None if o8 is None else _p(o8), int(trim_cells),
                                               C.byref(nv), C.byref(nf)))
        return self.poisson_last_mesh(int(nv.value), int(nf.value))

    # ---- smoothing and clean-up of the surface: meshlab.bat's script1 / script2 after the Poisson filter (csrc/k_meshclean.hip) ----
    @staticmethod
    def _mesh_clean_params(smooth_steps, cotangent, boundary, min_piece, relative, duplicates, zero_area, nonmanifold):
        prm = MeshCleanParams()
        prm.smooth_steps, prm.cotangent, prm.boundary = int(smooth_steps), int(bool(cotangent)), int(bool(boundary))
        prm.min_piece, prm.min_piece_relative = float(min_piece), int(bool(relative))
        prm.flags = ((_lib.MESH_CLEAN_DUPLICATES if duplicates else 0) | (_lib.MESH_CLEAN_ZERO_AREA if zero_area else 0)
                     | (_lib.MESH_CLEAN_NONMANIFOLD if nonmanifold else 0))
        return prm

    def _mesh_clean(self, fn, mesh_args, prm):
        """One of the three rsm_mesh_clean* entries: (n_vertices, n_faces, stats) of the mesh it leaves with the context."""
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.MESH_CLEAN_STATS)()
        self._chk(fn(self._h, *mesh_args, C.byref(prm), C.byref(nv), C.byref(nf), st))
        keys = ("n_vertices_in", "n_faces_in", "n_vertices", "n_faces", "border_vertices", "components", "components_removed", "removed_isolated",
                "removed_duplicate", "removed_zero_area", "removed_nonmanifold", "vertices_dropped")
        stats = {k: int(st[i]) for i, k in enumerate(keys)}
        stats["diameter"], stats["threshold"] = float(st[12]), float(st[13])
        return int(nv.value), int(nf.value), stats

    def mesh_clean(self, vertices, faces, smooth_steps=_MC["smooth_steps"], cotangent=_MC["cotangent"], boundary=_MC["boundary"],
                   min_piece=_MC["min_piece"], relative=_MC["relative"], duplicates=_MC["duplicates"], zero_area=_MC["zero_area"],
                   nonmanifold=_MC["nonmanifold"]):
        """What meshlab.bat does to the Poisson surface, on the GPU: script1's Laplacian smoothing (smooth_steps simultaneous steps, cotangent
        weights clamped at 0, border vertices smoothed along the border), then script2's removal of isolated pieces (components whose
        bounding-box diameter is below min_piece -- a fraction of the whole mesh's with relative=True, a length otherwise), duplicate
        faces, zero-area faces and faces on non-manifold edges, and of the vertices no face uses.  vertices [nv,3] float32, faces [nf,3]
        int32 -> (vertices, faces, stats dict).  The result is the context's last mesh (poisson_last_mesh[_device])."""
        v, f = _mesh_arrays(vertices, faces)
        prm = self._mesh_clean_params(smooth_steps, cotangent, boundary, min_piece, relative, duplicates, zero_area, nonmanifold)
        nv, nf, stats = self._mesh_clean(self._lib.rsm_mesh_clean, (_p(v), len(v), _p(f), len(f)), prm)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_clean_device(self, vertices_ptr, n_vertices, faces_ptr, n_faces, **kw):
        """rsm_mesh_clean_device on device buffers (addresses); keywords as mesh_clean.  Returns (n_vertices, n_faces, stats); the mesh
        stays with the context (poisson_last_mesh[_device] copies it out)."""
        prm = self._mesh_clean_params(**{**_MC, **kw})
        return self._mesh_clean(self._lib.rsm_mesh_clean_device, (vertices_ptr, n_vertices, faces_ptr, n_faces), prm)

    def mesh_clean_last(self, smooth_steps=_MC["smooth_steps"], cotangent=_MC["cotangent"], boundary=_MC["boundary"], min_piece=_MC["min_piece"],
                        relative=_MC["relative"], duplicates=_MC["duplicates"], zero_area=_MC["zero_area"], nonmanifold=_MC["nonmanifold"]):
        """mesh_clean of the context's last mesh (what poisson_mesh left) where it lies on the device; the result replaces it.
        Returns (vertices, faces, stats)."""
        prm = self._mesh_clean_params(smooth_steps, cotangent, boundary, min_piece, relative, duplicates, zero_area, nonmanifold)
        nv, nf, stats = self._mesh_clean(self._lib.rsm_mesh_clean_last, (), prm)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_smooth(self, vertices, faces, steps=5, cotangent=True, boundary=True, return_border=False):
        """Stage: the positions after `steps` smoothing steps (float32 [nv,3]; the faces are untouched); with return_border also the
        number of border vertices."""
        v, f = _mesh_arrays(vertices, faces)
        out = np.zeros((max(len(v), 1), 3), np.float32)
        nb = C.c_int64()
        self._chk(self._lib.rsm_stage_mesh_smooth(self._h, _p(v), len(v), _p(f), len(f), int(steps), int(bool(cotangent)), int(bool(boundary)),
                                                  _p(out), C.byref(nb)))
        out = out[:len(v)].copy()
        return (out, int(nb.value)) if return_border else out

    def mesh_components(self, faces, n_vertices):
        """Stage: (labels int32 [nf] = the lowest face index of each face's component, -1 for a face with a repeated index; the number of
        components).  Faces are connected across a shared edge, not across a shared vertex."""
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        lab = np.zeros(max(len(f), 1), np.int32)
        nc = C.c_int64()
        self._chk(self._lib.rsm_stage_mesh_components(self._h, _p(f), int(n_vertices), len(f), _p(lab), C.byref(nc)))
        return lab[:len(f)].copy(), int(nc.value)

    # ---- the density trim of the surface: mesh.bat's PoissonRecon --density + SurfaceTrimmer (csrc/k_meshtrim.hip) ----
    _TRIM_KEYS = ("n_vertices_in", "n_faces_in", "n_vertices", "n_faces", "n_valid", "n_invalid", "cut_edges", "faces_split", "repeated_index_faces",
                  "zero_area_triangles", "components_kept", "components_dropped", "moved_to_dropped", "moved_to_kept", "q_total")

    @classmethod
    def _trim_stats(cls, st):
        stats = {k: int(st[i]) for i, k in enumerate(cls._TRIM_KEYS)}
        stats.update(value_min=float(st[15]), value_max=float(st[16]), diagonal2=float(st[17]), density_step=float(st[18]), kernel_depth=int(st[19]))
        return stats

    @staticmethod
    def _samples(samples_xyz, samples_normals):
        xyz = np.ascontiguousarray(samples_xyz, np.float32).reshape(-1, 3)
        return xyz, None if samples_normals is None else _normals4(samples_normals, len(xyz))

    def _mesh_trim(self, fn, mesh_args, sample_args, depth, scale, kernel_depth, samples_per_node, smooth_steps, trim, island_ratio):
        """One of the three rsm_mesh_trim* entries: (n_vertices, n_faces, stats) of the mesh it leaves with the context."""
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.MESH_TRIM_STATS)()
        prm = MeshTrimParams(int(depth), float(scale), int(kernel_depth), float(samples_per_node), int(smooth_steps), float(trim), float(island_ratio))
        self._chk(fn(self._h, *mesh_args, *sample_args, C.byref(prm), C.byref(nv), C.byref(nf), st))
        return int(nv.value), int(nf.value), self._trim_stats(st)

    def mesh_trim(self, vertices, faces, samples_xyz, samples_normals=None, depth=9, scale=1.1, kernel_depth=_MT["kernel_depth"],
                  samples_per_node=_MT["samples_per_node"], smooth_steps=_MT["smooth_steps"], trim=_MT["trim"], island_ratio=_MT["island_ratio"]):
        """What mesh.bat's PoissonRecon --density and SurfaceTrimmer do to the surface, on the GPU: every vertex gets the depth at which a
        grid node would hold samples_per_node of the samples around it (a count splat on 2^kernel_depth nodes per axis of the box the
        Poisson call with this depth and scale used; 0 = depth - 2), the values are smoothed over the mesh smooth_steps times, the surface
        is cut along value = trim (crossing triangles are split) and pieces on either side of the cut below island_ratio of the whole area
        change side.  Call poisson_mesh with trim_cells=0 first.  vertices [nv,3] float32, faces [nf,3] int32, samples [n,3] float32 with
        normals [n,4] / [n,3] or None -> (vertices, faces, stats dict).  The result is the context's last mesh."""
        v, f = _mesh_arrays(vertices, faces)
        xyz, nrm = self._samples(samples_xyz, samples_normals)
        nv, nf, stats = self._mesh_trim(self._lib.rsm_mesh_trim, (_p(v), len(v), _p(f), len(f)), (_p(xyz), None if nrm is None else _p(nrm), len(xyz)), depth, scale,
                                        kernel_depth, samples_per_node, smooth_steps, trim, island_ratio)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_trim_device(self, vertices_ptr, n_vertices, faces_ptr, n_faces, samples_ptr, normals_ptr, n, depth=9, scale=1.1, **kw):
        """rsm_mesh_trim_device on device buffers (addresses; normals_ptr may be 0); keywords as mesh_trim.  Returns (n_vertices, n_faces,
        stats); the mesh stays with the context (poisson_last_mesh[_device] copies it out)."""
        return self._mesh_trim(self._lib.rsm_mesh_trim_device, (vertices_ptr, n_vertices, faces_ptr, n_faces), (samples_ptr, normals_ptr or None, n), depth, scale,
                               **{**_MT, **kw})

    def mesh_trim_last(self, samples_xyz, samples_normals=None, depth=9, scale=1.1, kernel_depth=_MT["kernel_depth"],
                       samples_per_node=_MT["samples_per_node"], smooth_steps=_MT["smooth_steps"], trim=_MT["trim"], island_ratio=_MT["island_ratio"]):
        """mesh_trim of the context's last mesh (what poisson_mesh left) where it lies on the device; the result replaces it.
        Returns (vertices, faces, stats)."""
        xyz, nrm = self._samples(samples_xyz, samples_normals)
        nv, nf, stats = self._mesh_trim(self._lib.rsm_mesh_trim_last, (), (_p(xyz), None if nrm is None else _p(nrm), len(xyz)), depth, scale, kernel_depth,
                                        samples_per_node, smooth_steps, trim, island_ratio)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_density(self, samples_xyz, samples_normals, points, depth, scale=1.1, kernel_depth=_MT["kernel_depth"], samples_per_node=_MT["samples_per_node"]):
        """Stage: the samples -> (rho float64 [m], value float64 [m], (valid, invalid)) at points [m,3] float32."""
        xyz, nrm = self._samples(samples_xyz, samples_normals)
        v = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        rho, val = np.zeros(max(len(v), 1), np.float64), np.zeros(max(len(v), 1), np.float64)
        counts = np.zeros(2, np.int64)
        prm = MeshTrimParams(int(depth), float(scale), int(kernel_depth), float(samples_per_node), 0, 0.0, 0.0)
        self._chk(self._lib.rsm_stage_mesh_density(self._h, _p(xyz), None if nrm is None else _p(nrm), len(xyz), C.byref(prm), _p(v), len(v), _p(rho), _p(val),
                                                   _p(counts)))
        return rho[:len(v)].copy(), val[:len(v)].copy(), (int(counts[0]), int(counts[1]))

    def mesh_value_smooth(self, values, faces, steps=_MT["smooth_steps"]):
        """Stage: a caller's values (float64 [nv]) after `steps` smoothing steps over the faces' incidences."""
        x = np.ascontiguousarray(values, np.float64).reshape(-1)
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        out = np.zeros(max(len(x), 1), np.float64)
        self._chk(self._lib.rsm_stage_mesh_value_smooth(self._h, _p(f), len(x), len(f), _p(x), int(steps), _p(out)))
        return out[:len(x)].copy()

    def mesh_split(self, vertices, faces, values, trim=_MT["trim"], island_ratio=0.0):
        """Stage: a caller's values (float64 [nv]) -> (vertices, faces, src_face int32 [nf'], side int32 [nf'] before the island rule,
        label int32 [nf'], stats) of the mesh cut along value = trim."""
        v, f = _mesh_arrays(vertices, faces)
        x = np.ascontiguousarray(values, np.float64).reshape(-1)
        assert len(x) == len(v)
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.MESH_TRIM_STATS)()
        info = [np.zeros(max(3 * len(f), 1), np.int32) for _ in range(3)]
        self._chk(self._lib.rsm_stage_mesh_split(self._h, _p(v), len(v), _p(f), len(f), _p(x), float(trim), float(island_ratio), C.byref(nv), C.byref(nf), st,
                                                 *(_p(a) for a in info)))
        ov, of = self.poisson_last_mesh(int(nv.value), int(nf.value))
        return (ov, of) + tuple(a[:len(of)].copy() for a in info) + (self._trim_stats(st),)

    # ---- the closing of the surface's small holes: script2.mlx's "Close Holes" (csrc/k_meshclose.hip) ----
    _CLOSE_KEYS = ("n_vertices_in", "n_faces_in", "n_faces", "border_entries", "components", "loops", "open_components", "loops_closed", "loops_too_long",
                   "lone_triangles", "loops_untriangulated", "faces_added", "longest_closed", "longest_loop")

    def _mesh_close(self, fn, mesh_args, max_hole_size):
        """One of the three rsm_mesh_close_holes* entries: (n_vertices, n_faces, stats) of the mesh it leaves with the context."""
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.MESH_CLOSE_STATS)()
        prm = MeshCloseParams(int(max_hole_size))
        self._chk(fn(self._h, *mesh_args, C.byref(prm), C.byref(nv), C.byref(nf), st))
        return int(nv.value), int(nf.value), {k: int(st[i]) for i, k in enumerate(self._CLOSE_KEYS)}

    def mesh_close_holes(self, vertices, faces, max_hole_size=30):
        """script2.mlx's last filter, "Close Holes", on the GPU: every border loop of at most max_hole_size (3..64) edges whose vertices all
        have one border edge in and one out, other than the border of a lone triangle, is filled with the least-area triangulation of its
        ring that uses no edge the mesh already has and no triangle without area; bow-ties, borders between faces
        oriented against each other and longer loops stay.  vertices [nv,3] float32, faces [nf,3] int32 -> (vertices: the input's, faces:
        the input's followed by the new ones, stats dict).  The result is the context's last mesh (poisson_last_mesh[_device])."""
        v, f = _mesh_arrays(vertices, faces)
        nv, nf, stats = self._mesh_close(self._lib.rsm_mesh_close_holes, (_p(v), len(v), _p(f), len(f)), max_hole_size)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_close_holes_device(self, vertices_ptr, n_vertices, faces_ptr, n_faces, max_hole_size=30):
        """rsm_mesh_close_holes_device on device buffers (addresses).  Returns (n_vertices, n_faces, stats); the mesh stays with the context
        (poisson_last_mesh[_device] copies it out)."""
        return self._mesh_close(self._lib.rsm_mesh_close_holes_device, (vertices_ptr, n_vertices, faces_ptr, n_faces), max_hole_size)

    def mesh_close_holes_last(self, max_hole_size=30):
        """mesh_close_holes of the context's last mesh (what poisson_mesh / mesh_trim / mesh_clean left) where it lies on the device; the
        result replaces it and its colours are dropped.  Returns (vertices, faces, stats)."""
        nv, nf, stats = self._mesh_close(self._lib.rsm_mesh_close_holes_last, (), max_hole_size)
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_border_loops(self, faces, n_vertices):
        """Stage: per entry 3 f + j (labels int32 [3 nf] = the lowest entry of its border component, -1 where the edge is no border; sizes
        int32 [3 nf] = L for a loop's entries, 0 for an open component's, -1 otherwise; the number of border components)."""
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        lab = np.zeros(max(3 * len(f), 1), np.int32)
        size = np.zeros(max(3 * len(f), 1), np.int32)
        nc = C.c_int64()
        self._chk(self._lib.rsm_stage_mesh_border_loops(self._h, _p(f), int(n_vertices), len(f), _p(lab), _p(size), C.byref(nc)))
        return lab[:3 * len(f)].copy(), size[:3 * len(f)].copy(), int(nc.value)

    def mesh_hole_triangulate(self, ring_xyz, forbidden=None):
        """Stage: a ring of L (3..64) float32 points and, optionally, an L x L array of forbidden pairs (read at [i, j], i + 2 <= j) ->
        (W(0, L-1) float, triangles int32 [L-2, 3] of ring positions in the order of the output); (inf, [0, 3]) when the ring has no
        admissible triangulation."""
        r = np.ascontiguousarray(ring_xyz, np.float32).reshape(-1, 3)
        L = len(r)
        m = None if forbidden is None else np.ascontiguousarray(np.asarray(forbidden) != 0, np.uint8)
        assert m is None or m.shape == (L, L)
        tri = np.zeros((max(L - 2, 1), 3), np.int32)
        w, nt = C.c_double(), C.c_int()
        self._chk(self._lib.rsm_stage_hole_triangulate(self._h, _p(r), L, None if m is None else _p(m), C.byref(w), _p(tri), C.byref(nt)))
        return float(w.value), tri[:int(nt.value)].copy()

    # ---- the decimation of the final mesh: decimation.mlx's "Quadric Edge Collapse Decimation" (csrc/k_meshdecimate.hip) ----
    _DECIMATE_KEYS = ("n_vertices_in", "n_faces_in", "n_vertices", "n_faces", "repeated_index_faces", "rounds", "collapses", "border_collapses",
                      "rejected_nonmanifold", "rejected_locked", "rejected_link", "rejected_border", "rejected_duplicate", "rejected_normal",
                      "rejected_not_finite", "locked_vertices", "max_valence", "max_cost", "target_reached", "target")

    @staticmethod
    def mesh_decimate_params(target_faces=100000, target_fraction=0.0, quality_thr=0.3, preserve_boundary=False, boundary_weight=1.0, preserve_normal=False,
                             preserve_topology=True, optimal_placement=True, min_error=1e-15, max_rounds=1000):
        """rsm_mesh_decimate_params with decimation.mlx's values as defaults (min_error: VCG's floor; max_rounds: DESIGN.md 9 f13)."""
        return MeshDecimateParams(int(target_faces), float(target_fraction), float(quality_thr), int(preserve_boundary), float(boundary_weight),
                                  int(preserve_normal), int(preserve_topology), int(optimal_placement), float(min_error), int(max_rounds))

    def _mesh_decimate(self, fn, mesh_args, prm):
        """One of the three rsm_mesh_decimate* entries: (n_vertices, n_faces, stats) of the mesh it leaves with the context."""
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.MESH_DECIMATE_STATS)()
        self._chk(fn(self._h, *mesh_args, C.byref(prm), C.byref(nv), C.byref(nf), st))
        return int(nv.value), int(nf.value), {k: (float(st[i]) if k == "max_cost" else int(st[i])) for i, k in enumerate(self._DECIMATE_KEYS)}

    def mesh_decimate(self, vertices, faces, **params):
        """decimation.mlx's "Quadric Edge Collapse Decimation" on the GPU: rounds of independent edge collapses in the order
        of their quadric error over the clamped shape quality, until the mesh has target_faces (or target_fraction of its) faces or no edge
        may collapse; then the vertices no face refers to go.  params: mesh_decimate_params'.  vertices [nv,3] float32, faces [nf,3] int32 ->
        (vertices, faces, stats dict).  The result is the context's last mesh (poisson_last_mesh[_device])."""
        v, f = _mesh_arrays(vertices, faces)
        nv, nf, stats = self._mesh_decimate(self._lib.rsm_mesh_decimate, (_p(v), len(v), _p(f), len(f)), self.mesh_decimate_params(**params))
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_decimate_device(self, vertices_ptr, n_vertices, faces_ptr, n_faces, **params):
        """rsm_mesh_decimate_device on device buffers (addresses).  Returns (n_vertices, n_faces, stats); the mesh stays with the context
        (poisson_last_mesh[_device] copies it out)."""
        return self._mesh_decimate(self._lib.rsm_mesh_decimate_device, (vertices_ptr, n_vertices, faces_ptr, n_faces), self.mesh_decimate_params(**params))

    def mesh_decimate_last(self, **params):
        """mesh_decimate of the context's last mesh where it lies on the device; the result replaces it and its colours are dropped.
        Returns (vertices, faces, stats)."""
        nv, nf, stats = self._mesh_decimate(self._lib.rsm_mesh_decimate_last, (), self.mesh_decimate_params(**params))
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_quadrics(self, vertices, faces, boundary_weight=1.0):
        """Stage: the quadric of every vertex, float64 [nv,10] (xx xy xz xd yy yz yd zz zd dd)."""
        v, f = _mesh_arrays(vertices, faces)
        q = np.zeros((max(len(v), 1), 10), np.float64)
        self._chk(self._lib.rsm_stage_mesh_quadrics(self._h, _p(v), len(v), _p(f), len(f), float(boundary_weight), _p(q)))
        return q[:len(v)].copy()

    def mesh_collapse_costs(self, vertices, faces, quadrics, **params):
        """Stage: per unique edge in key order (keys uint64 = (a << 32) | b, multiplicity int32, cost float64 with +inf for no candidate,
        reject int32 -- bits 0-3 why, bits 4-5 the placement branch --, position float32 [ne,3])."""
        v, f = _mesh_arrays(vertices, faces)
        q = np.ascontiguousarray(quadrics, np.float64).reshape(-1, 10)
        assert len(q) == len(v)
        n = max(3 * len(f), 1)
        key, mult, cost, rej, pos = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
        ne = C.c_int64()
        prm = self.mesh_decimate_params(**params)
        self._chk(self._lib.rsm_stage_mesh_collapse_costs(self._h, _p(v), len(v), _p(f), len(f), _p(q), C.byref(prm), _p(key), _p(mult), _p(cost), _p(rej), _p(pos),
                                                          C.byref(ne)))
        ne = int(ne.value)
        return tuple(a[:ne].copy() for a in (key, mult, cost, rej, pos))

    def mesh_collapse_round(self, vertices, faces, quadrics, need, **params):
        """Stage: one round that is to remove `need` faces -> (vertices float32 [nv,3], faces int32 [nf',3], quadrics float64 [nv,10], the
        selected keys uint64 in priority order, the number of them that were collapsed)."""
        v, f = _mesh_arrays(vertices, faces)
        q = np.ascontiguousarray(quadrics, np.float64).reshape(-1, 10)
        assert len(q) == len(v)
        ov, oq = np.zeros((max(len(v), 1), 3), np.float32), np.zeros((max(len(v), 1), 10), np.float64)
        of, sel = np.zeros((max(len(f), 1), 3), np.int32), np.zeros(max(3 * len(f), 1), np.uint64)
        nfo, nsel, nkept = C.c_int64(), C.c_int64(), C.c_int64()
        prm = self.mesh_decimate_params(**params)
        self._chk(self._lib.rsm_stage_mesh_collapse_round(self._h, _p(v), len(v), _p(f), len(f), _p(q), C.byref(prm), int(need), _p(ov), _p(of), _p(oq),
                                                          C.byref(nfo), _p(sel), C.byref(nsel), C.byref(nkept)))
        return ov[:len(v)].copy(), of[:int(nfo.value)].copy(), oq[:len(v)].copy(), sel[:int(nsel.value)].copy(), int(nkept.value)

    # ---- the subdivision of the final mesh: subdiv.mlx's "Subdivision Surfaces: Loop" (csrc/k_meshsubdivide.hip) ----
    _SUBDIVIDE_KEYS = ("n_vertices_in", "n_faces_in", "n_vertices", "n_faces", "iterations", "threshold", "split_edges", "split_border_edges",
                       "split_many_face_edges", "faces_0_splits", "faces_1_split", "faces_2_splits", "faces_3_splits", "moved_interior", "moved_border",
                       "locked_vertices", "max_valence")

    @staticmethod
    def mesh_subdivide_params(iterations=3, threshold=0.0, threshold_fraction=0.0, weight_scheme=0):
        """rsm_mesh_subdivide_params.  threshold_fraction > 0: the threshold is that fraction of the input's box diagonal (subdiv.mlx: 0.01)
        and `threshold` is not read; both 0: every edge splits.  weight_scheme: only 0 (Loop's own weights) is built."""
        return MeshSubdivideParams(int(iterations), float(threshold), float(threshold_fraction), int(weight_scheme))

    def _mesh_subdivide(self, fn, mesh_args, prm):
        """One of the three rsm_mesh_subdivide* entries: (n_vertices, n_faces, stats) of the mesh it leaves with the context."""
        nv, nf = C.c_int64(), C.c_int64()
        st = (C.c_double * _lib.MESH_SUBDIVIDE_STATS)()
        self._chk(fn(self._h, *mesh_args, C.byref(prm), C.byref(nv), C.byref(nf), st))
        return int(nv.value), int(nf.value), {k: (float(st[i]) if k == "threshold" else int(st[i])) for i, k in enumerate(self._SUBDIVIDE_KEYS)}

    def mesh_subdivide(self, vertices, faces, **params):
        """subdiv.mlx's "Subdivision Surfaces: Loop" on the GPU: per iteration every edge strictly longer than the threshold
        gets a new vertex, the old vertices at such an edge move by Loop's rules, every face becomes 1 to 4.  Loop's own weights only
        (MeshLab's LoopWeight 0); positions only -- no colours are carried across.  params: mesh_subdivide_params'.  vertices [nv,3]
        float32, faces [nf,3] int32 -> (vertices, faces, stats dict).  The result is the context's last mesh (poisson_last_mesh[_device])."""
        v, f = _mesh_arrays(vertices, faces)
        nv, nf, stats = self._mesh_subdivide(self._lib.rsm_mesh_subdivide, (_p(v), len(v), _p(f), len(f)), self.mesh_subdivide_params(**params))
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_subdivide_device(self, vertices_ptr, n_vertices, faces_ptr, n_faces, **params):
        """rsm_mesh_subdivide_device on device buffers (addresses).  Returns (n_vertices, n_faces, stats); the mesh stays with the context
        (poisson_last_mesh[_device] copies it out)."""
        return self._mesh_subdivide(self._lib.rsm_mesh_subdivide_device, (vertices_ptr, n_vertices, faces_ptr, n_faces), self.mesh_subdivide_params(**params))

    def mesh_subdivide_last(self, **params):
        """mesh_subdivide of the context's last mesh where it lies on the device; the result replaces it and its colours are dropped.
        Returns (vertices, faces, stats)."""
        nv, nf, stats = self._mesh_subdivide(self._lib.rsm_mesh_subdivide_last, (), self.mesh_subdivide_params(**params))
        return self.poisson_last_mesh(nv, nf) + (stats,)

    def mesh_subdivide_edges(self, vertices, faces, **params):
        """Stage: the decisions of one iteration -> dict(keys uint64 = (a << 32) | b per unique edge in key order, multiplicity int32, split
        int32 0 / 1, odd float32 [ne,3] (zeros where the edge stays), vertex_class int32 [nv] (0 interior, 1 border, 2 locked), even float32
        [nv,3], threshold float)."""
        v, f = _mesh_arrays(vertices, faces)
        n = max(3 * len(f), 1)
        key, mult, split, odd = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32)
        cls, even = np.zeros(max(len(v), 1), np.int32), np.zeros((max(len(v), 1), 3), np.float32)
        ne, thr = C.c_int64(), C.c_double()
        prm = self.mesh_subdivide_params(**params)
        self._chk(self._lib.rsm_stage_mesh_subdivide_edges(self._h, _p(v), len(v), _p(f), len(f), C.byref(prm), _p(key), _p(mult), _p(split), _p(odd), C.byref(ne),
                                                           _p(cls), _p(even), C.byref(thr)))
        ne = int(ne.value)
        return dict(keys=key[:ne].copy(), multiplicity=mult[:ne].copy(), split=split[:ne].copy(), odd=odd[:ne].copy(), vertex_class=cls[:len(v)].copy(),
                    even=even[:len(v)].copy(), threshold=float(thr.value))

    # ---- colours of the mesh from the rig's views, where run() calls TextureStitcher (csrc/k_meshcolor.hip) ----
    @staticmethod
    def mesh_color_views(cams):
        """rsm_dedup_view per pair from cam[i][0..1] (Camera objects: P, image and, optionally, mask) as the colouring reads them: bound and
        CamCenter are not used, a mask of None means all 255.  Returns (ctypes array, arrays to keep alive during the call)."""
        return _views(cams, "mesh_color", False)

    def _mesh_color(self, fn, mesh_args, cams, out_args, depth_eps, mode, min_cos):
        """One of the three rsm_mesh_color* entries over the views of cams: the stats."""
        views, keep = self.mesh_color_views(cams)
        st = (C.c_double * _lib.MESH_COLOR_STATS)()
        prm = MeshColorParams(int(mode), float(min_cos), float(depth_eps))
        self._chk(fn(self._h, *mesh_args, views, len(cams), C.byref(prm), *out_args, st))
        del keep
        return {k: int(st[i]) for i, k in enumerate(("n_vertices", "coloured", "no_normal", "visible_views", "items_drawn", "items_big_box"))}

    def mesh_color(self, vertices, faces, cams, depth_eps, mode=1, min_cos=0.2):
        """Colours of a host mesh from the views of cams (m_ImageData.cam: per pair two cameras with P, image, mask), where
        CCloudOptimization::run calls TextureStitcher.  The views are numbered every pair's view 0, then every pair's view 1.  A vertex is
        visible in a view when it is in front of it, projects (texture_color's pixel) inside the image onto mask 255, its normal makes
        cos > min_cos with the direction to the camera centre, and the view's depth buffer of the mesh holds no surface more than
        depth_eps (scene units) in front of it.  mode 0: the colour of the visible view of largest cos; 1: the cos-weighted blend.
        Returns (rgb uint8 [nv,3]: red, green, blue, (127, 127, 127) where no view sees the vertex; best_view int32 [nv], -1 there;
        stats dict)."""
        v, f = _mesh_arrays(vertices, faces)
        rgb = np.zeros((max(len(v), 1), 3), np.uint8)
        best = np.zeros(max(len(v), 1), np.int32)
        stats = self._mesh_color(self._lib.rsm_mesh_color, (_p(v), len(v), _p(f), len(f)), cams, (_p(rgb), _p(best)), depth_eps, mode, min_cos)
        return rgb[:len(v)].copy(), best[:len(v)].copy(), stats

    def mesh_color_device(self, vertices_ptr, n_vertices, faces_ptr, n_faces, cams, rgb_ptr, best_view_ptr, depth_eps, mode=1, min_cos=0.2):
        """rsm_mesh_color_device on device buffers (addresses; best_view_ptr may be 0); the views' images stay on the host.  Returns stats."""
        return self._mesh_color(self._lib.rsm_mesh_color_device, (vertices_ptr, n_vertices, faces_ptr, n_faces), cams, (rgb_ptr, best_view_ptr), depth_eps, mode, min_cos)

    def mesh_color_last(self, cams, depth_eps, mode=1, min_cos=0.2):
        """mesh_color of the context's last mesh (what poisson_mesh / mesh_clean left) where it lies on the device; the mesh is untouched.
        Returns (rgb, best_view, stats)."""
        stats = self._mesh_color(self._lib.rsm_mesh_color_last, (), cams, (), depth_eps, mode, min_cos)
        nv = stats["n_vertices"]
        rgb = np.zeros((max(nv, 1), 3), np.uint8)
        best = np.zeros(max(nv, 1), np.int32)
        self._chk(self._lib.rsm_mesh_last_colors(self._h, _p(rgb), _p(best)))
        return rgb[:nv].copy(), best[:nv].copy(), stats

    # ---- the views' exposure seams levelled in those colours (csrc/k_meshstitch.hip) ----
    _STITCH_KEYS = ("n_vertices", "coloured", "incidences", "seam_incidences", "seam_two_terms", "seam_one_term", "seam_no_term", "dmax", "steps")

    def _mesh_stitch(self, fn, mesh_args, cams, out_args, depth_eps, min_cos, lam, iterations, reduction, seam_gradient):
        """One of the three rsm_mesh_stitch* entries over the views of cams: the stats."""
        views, keep = self.mesh_color_views(cams)
        st = (C.c_double * _lib.MESH_STITCH_STATS)()
        prm = MeshColorParams(0, float(min_cos), float(depth_eps))
        sp = MeshStitchParams(float(lam), int(iterations), float(reduction), int(seam_gradient))
        self._chk(fn(self._h, *mesh_args, views, len(cams), C.byref(prm), C.byref(sp), *out_args, st))
        del keep
        stats = {k: int(st[i]) for i, k in enumerate(self._STITCH_KEYS)}
        stats.update(rel_residual=float(st[9]), max_change=float(st[10]), clamped=int(st[11]))
        return stats

    def mesh_stitch(self, vertices, faces, cams, depth_eps, min_cos=0.2, lam=0.01, iterations=0, reduction=1e-4, seam_gradient=True):
        """mesh_color's best-view colours (mode 0) of a host mesh with the views' exposure seams levelled, the other half of
        TextureStitcher's job: per channel the screened gradient-domain system over the coloured vertices -- inside a
        view the colours' own differences are kept, across a seam the views' own differences where they see both ends
        (seam_gradient=False: 0), and lam pulls towards the colouring, so that a view's offset decays over about 1 / sqrt(lam) edges.
        iterations Chebyshev steps, or with 0 as many as bring the error down to `reduction` of the start's.  Returns (rgb uint8 [nv,3],
        best_view int32 [nv], stats dict); uncoloured vertices stay (127, 127, 127)."""
        v, f = _mesh_arrays(vertices, faces)
        rgb = np.zeros((max(len(v), 1), 3), np.uint8)
        best = np.zeros(max(len(v), 1), np.int32)
        stats = self._mesh_stitch(self._lib.rsm_mesh_stitch, (_p(v), len(v), _p(f), len(f)), cams, (_p(rgb), _p(best)), depth_eps, min_cos, lam, iterations,
                                  reduction, seam_gradient)
        return rgb[:len(v)].copy(), best[:len(v)].copy(), stats

    def mesh_stitch_device(self, vertices_ptr, n_vertices, faces_ptr, n_faces, cams, rgb_ptr, best_view_ptr, depth_eps, min_cos=0.2, lam=0.01, iterations=0,
                           reduction=1e-4, seam_gradient=True):
        """rsm_mesh_stitch_device on device buffers (addresses; best_view_ptr may be 0); the views' images stay on the host.  Returns stats."""
        return self._mesh_stitch(self._lib.rsm_mesh_stitch_device, (vertices_ptr, n_vertices, faces_ptr, n_faces), cams, (rgb_ptr, best_view_ptr), depth_eps,
                                 min_cos, lam, iterations, reduction, seam_gradient)

    def mesh_stitch_last(self, cams, depth_eps, min_cos=0.2, lam=0.01, iterations=0, reduction=1e-4, seam_gradient=True):
        """mesh_stitch of the context's last mesh where it lies on the device; the mesh is untouched and the colours stay with the context
        as mesh_color_last's do.  Returns (rgb, best_view, stats)."""
        stats = self._mesh_stitch(self._lib.rsm_mesh_stitch_last, (), cams, (), depth_eps, min_cos, lam, iterations, reduction, seam_gradient)
        nv = stats["n_vertices"]
        rgb = np.zeros((max(nv, 1), 3), np.uint8)
        best = np.zeros(max(nv, 1), np.int32)
        self._chk(self._lib.rsm_mesh_last_colors(self._h, _p(rgb), _p(best)))
        return rgb[:nv].copy(), best[:nv].copy(), stats

    def mesh_visibility(self, vertices, faces, cams, depth_eps, min_cos=0.2):
        """Stage: per vertex the mask of the views that see it (uint64 [nv], bit v = view v), by the colouring's visibility test."""
        v, f = _mesh_arrays(vertices, faces)
        views, keep = self.mesh_color_views(cams)
        vis = np.zeros(max(len(v), 1), np.uint64)
        prm = MeshColorParams(0, float(min_cos), float(depth_eps))
        self._chk(self._lib.rsm_stage_mesh_visibility(self._h, _p(v), len(v), _p(f), len(f), views, len(cams), C.byref(prm), _p(vis)))
        del keep
        return vis[:len(v)].copy()

    def mesh_stitch_rhs(self, vertices, faces, cams, rgb, best_view, vis, seam_gradient=True):
        """Stage: a caller's colouring (rgb uint8 [nv,3], best_view int32 [nv], vis uint64 [nv]) -> (G float64 [nv,3], deg int32 [nv],
        counts dict: incidences, seam_incidences, seam_two_terms, seam_one_term, seam_no_term)."""
        v, f = _mesh_arrays(vertices, faces)
        n = len(v)
        views, keep = self.mesh_color_views(cams)
        c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        b = np.ascontiguousarray(best_view, np.int32).reshape(-1)
        m = np.ascontiguousarray(vis, np.uint64).reshape(-1)
        assert len(c) == n and len(b) == n and len(m) == n
        G = np.zeros((max(n, 1), 3), np.float64)
        deg = np.zeros(max(n, 1), np.int32)
        counts = np.zeros(5, np.int64)
        self._chk(self._lib.rsm_stage_mesh_stitch_rhs(self._h, _p(v), n, _p(f), len(f), views, len(cams), _p(c), _p(b), _p(m), int(bool(seam_gradient)),
                                                      _p(G), _p(deg), _p(counts)))
        del keep
        return G[:n].copy(), deg[:n].copy(), {k: int(counts[i]) for i, k in enumerate(self._STITCH_KEYS[2:7])}

    def mesh_stitch_solve(self, faces, best_view, rgb, G, lam, iterations):
        """Stage: `iterations` Chebyshev steps from a caller's best_view (its sign alone counts), rgb and G -> (x float64 [nv,3], the
        relative residual after them)."""
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        b = np.ascontiguousarray(best_view, np.int32).reshape(-1)
        n = len(b)
        c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        g = np.ascontiguousarray(G, np.float64).reshape(-1, 3)
        assert len(c) == n and len(g) == n
        x = np.zeros((max(n, 1), 3), np.float64)
        rel = C.c_double()
        self._chk(self._lib.rsm_stage_mesh_stitch_solve(self._h, _p(f), n, len(f), _p(b), _p(c), _p(g), float(lam), int(iterations), _p(x), C.byref(rel)))
        return x[:n].copy(), float(rel.value)

    # ---- the vertices no view sees filled from the colours around them (csrc/k_meshfill.hip) ----
    _FILL_KEYS = ("n_vertices", "known", "filled", "unreached", "rounds", "incidences", "dmax", "steps", "clamped")

    def _mesh_fill(self, fn, args, max_rounds, iterations, reduction):
        """One of the three rsm_mesh_fill_colors* entries: the stats."""
        st = (C.c_double * _lib.MESH_FILL_STATS)()
        prm = MeshFillParams(int(max_rounds), int(iterations), float(reduction))
        self._chk(fn(self._h, *args, C.byref(prm), st))
        stats = {k: int(st[i]) for i, k in enumerate(self._FILL_KEYS)}
        stats.update(max_change=float(st[9]))
        return stats

    def mesh_fill_colors(self, faces, rgb, best_view, max_rounds=0, iterations=0, reduction=1e-4):
        """The colours of a mesh (mesh_color's or mesh_stitch's rgb uint8 [nv,3] and best_view int32 [nv]) with every uncoloured vertex
        (best_view < 0) that is connected to a coloured one filled by the harmonic extension of the colours around it on the mesh graph
        (DESIGN.md 9 f18): a front of means gives the start and each vertex's level (its distance in edges from the coloured ones, at most
        max_rounds when that is > 0), `iterations` Chebyshev steps -- or with 0 as many as bring the error down to `reduction` of the
        start's -- solve the system.  Coloured vertices keep their bytes.  Returns (rgb uint8 [nv,3], level int32 [nv]: 0 coloured,
        1 .. rounds filled, -1 left as it was; stats dict)."""
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        b = np.ascontiguousarray(best_view, np.int32).reshape(-1)
        n = len(b)
        c = np.array(rgb, np.uint8).reshape(-1, 3)
        assert len(c) == n
        c = np.ascontiguousarray(np.concatenate([c, np.zeros((1, 3), np.uint8)]))
        level = np.zeros(max(n, 1), np.int32)
        stats = self._mesh_fill(self._lib.rsm_mesh_fill_colors, (_p(f), n, len(f), _p(c), _p(b), _p(level)), max_rounds, iterations, reduction)
        return c[:n].copy(), level[:n].copy(), stats

    def mesh_fill_colors_device(self, faces_ptr, n_vertices, n_faces, rgb_ptr, best_view_ptr, level_ptr=0, max_rounds=0, iterations=0, reduction=1e-4):
        """rsm_mesh_fill_colors_device on device buffers (addresses; rgb in and out; level_ptr may be 0).  Returns stats."""
        return self._mesh_fill(self._lib.rsm_mesh_fill_colors_device, (faces_ptr, n_vertices, n_faces, rgb_ptr, best_view_ptr, level_ptr or None), max_rounds,
                               iterations, reduction)

    def mesh_fill_colors_last(self, max_rounds=0, iterations=0, reduction=1e-4):
        """mesh_fill_colors of the context's last mesh and the colours mesh_color_last / mesh_stitch_last left with it, where they lie on
        the device (RsmError RSM_E_STATE when it has none).  Returns (rgb, best_view, stats): best_view is unchanged, a filled vertex
        keeps -1."""
        stats = self._mesh_fill(self._lib.rsm_mesh_fill_colors_last, (), max_rounds, iterations, reduction)
        nv = stats["n_vertices"]
        rgb = np.zeros((max(nv, 1), 3), np.uint8)
        best = np.zeros(max(nv, 1), np.int32)
        self._chk(self._lib.rsm_mesh_last_colors(self._h, _p(rgb), _p(best)))
        return rgb[:nv].copy(), best[:nv].copy(), stats

    def mesh_fill_front(self, faces, rgb, best_view, max_rounds=0, round_batch=0):
        """Stage: the front alone -> (x float64 [nv,3]: the bytes as doubles where it wrote nothing, level int32 [nv]: -1 unreached, L).
        round_batch: the rounds launched between two read-backs of the largest level (0: the library's 16); the result does not depend on it."""
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        b = np.ascontiguousarray(best_view, np.int32).reshape(-1)
        n = len(b)
        c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        assert len(c) == n
        x = np.zeros((max(n, 1), 3), np.float64)
        level = np.zeros(max(n, 1), np.int32)
        L = C.c_int()
        self._chk(self._lib.rsm_stage_mesh_fill_front(self._h, _p(f), n, len(f), _p(c), _p(b), int(max_rounds), int(round_batch), _p(x), _p(level), C.byref(L)))
        return x[:n].copy(), level[:n].copy(), int(L.value)

    def mesh_fill_solve(self, faces, x, level, L, iterations):
        """Stage: `iterations` Chebyshev steps from a caller's x float64 [nv,3], level (0 known, 1 .. L filled, anything else unreached)
        and L -> x float64 [nv,3]; only filled rows change."""
        f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
        lv = np.ascontiguousarray(level, np.int32).reshape(-1)
        n = len(lv)
        xx = np.array(x, np.float64).reshape(-1, 3)
        assert len(xx) == n
        xx = np.ascontiguousarray(np.concatenate([xx, np.zeros((1, 3))]))
        self._chk(self._lib.rsm_stage_mesh_fill_solve(self._h, _p(f), n, len(f), _p(lv), int(L), int(iterations), _p(xx)))
        return xx[:n].copy()

    def texture_color(self, xyz, P, image):
        """Stage: texture_color (CCloudOptimization.cpp:400-421) of xyz [n,3] float32 against one view (P 3x4, image BGR uint8 [H,W,3]):
        rgb uint8 [n,3], (127, 127, 127) outside the image."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        P = np.ascontiguousarray(P, np.float64).reshape(12)
        img = _u8(image)
        rgb = np.zeros((max(len(xyz), 1), 3), np.uint8)
        self._chk(self._lib.rsm_texture_color(self._h, _p(xyz), len(xyz), _p(P), _p(img), int(img.shape[1]), int(img.shape[0]), _p(rgb)))
        return rgb[:len(xyz)].copy()

    def mesh_depth(self, vertices, faces, P, width, height):
        """Stage: one view's depth buffer of the mesh, uint32 [height,width]: the largest float32 bit pattern of the inverse depth drawn at
        each pixel centre (0: nothing drawn)."""
        v, f = _mesh_arrays(vertices, faces)
        P = np.ascontiguousarray(P, np.float64).reshape(12)
        w = np.zeros((max(int(height), 1), max(int(width), 1)), np.uint32)
        self._chk(self._lib.rsm_stage_mesh_depth(self._h, _p(v), len(v), _p(f), len(f), _p(P), int(width), int(height), _p(w)))
        return w
