"""python -m reconstruction_amd <config.yml> [--device N] [--out cloud.ply] [--filter] [--outrem [NEIGHBOURS RADIUS]]
                              [--mls [--isdelete] [--mls-out bigcloud.ply]]
                              [--mesh [--mesh-depth 9] [--mesh-trim 4] [--mesh-band [B] [--mesh-band-samples-per-node [3]]] [--mesh-out bigmesh.ply]
                               [--mesh-samples-per-node [2] [--mesh-kernel-depth 0]]
                               [--mesh-density-trim [7] [--mesh-density-smooth 100] [--mesh-island-ratio 0.01]]
                               [--mesh-clean [--mesh-smooth 5] [--mesh-min-piece 10%]] [--mesh-close-holes [30]] [--mesh-decimate [100000]]
                               [--mesh-subdivide [3] [--mesh-subdivide-threshold 1]]
                               [--mesh-color [--mesh-color-mode blend] [--mesh-color-min-cos 0.2] [--mesh-color-eps LENGTH]]
                               [--mesh-stitch [--mesh-stitch-lambda 0.01] [--mesh-stitch-iterations 0]] [--mesh-color-fill [ROUNDS]]]

The command-line shape of the reference's main() (reconstruction/main.cpp:5-23) for the part this package covers:
CReconstrction::Init (configuration + calibration, CReconstruction.cpp:5-19) -> CStereoMatching::MatchAllLayer
(Rectify, pyramid, matching, refinement, cloud; on the MI355X) -> per pair CCloudOptimization::filter's outlier removal
and normals (--filter; CCloudOptimization.cpp:82-121, on the GPU) -> the merged point cloud as a PLY file -> with --mls
(implies --filter) the moving-least-squares block of CCloudOptimization::run (CCloudOptimization.cpp:348-389, on the GPU):
the smoothed, oriented cloud as bigcloud.ply (pcl::PointNormal, savePLYFileBinary), what the mesher reads; --isdelete runs the
multi-view duplicate deletion before it (CCloudOptimization.cpp:152-346, on the GPU).
With --outrem (implies --filter) the filter also runs the pcl::RadiusOutlierRemoval the reference has, commented out, between its outlier removal
and its normals (CCloudOptimization.cpp:90-96, on the GPU): a survivor stays only with more than NEIGHBOURS survivors within RADIUS of it (50 and 2
when given bare, CReconstruction.cpp:18's values).
With --mesh (implies --mls) the surface of that cloud: unscreened Poisson reconstruction on a dense grid and a trim, on the GPU,
where CCloudOptimization::run calls meshlab.bat's Poisson filter -> bigmesh.ply (not a bit-parity port of that tool: DESIGN.md 9 f7).
With --mesh-samples-per-node (implies --mesh) the Poisson call spreads every sample by the density of the cloud around it, as PoissonRecon's
--samplesPerNode does (2 when given bare, mesh.bat's value; script1.mlx uses 3), so that thinly sampled parts hold their place.
With --mesh-band (implies --mesh) the surface is one level finer than the dense grid reaches: --mesh-depth 6..10 is then the finest depth, a level
that exists only on a band of bricks around the points, on top of the dense solve one depth coarser (script1.mlx's OctDepth 10).
With --mesh-band-samples-per-node (implies --mesh-band 1) the banded call uses the density-adaptive splat: script1.mlx's OctDepth 10 and
SamplesPerNode 3 together.  --mesh-band with --mesh-samples-per-node stays refused, which is why this switch is its own.
With --mesh-density-trim (implies --mesh) the Poisson call runs without its occupancy trim and the surface is trimmed as mesh.bat's
SurfaceTrimmer does, on the GPU: cut along the iso-line of the smoothed sample density, small islands moved across.
With --mesh-clean (implies --mesh) bigmesh.ply is that surface after meshlab.bat's other filters, on the GPU: Laplacian smoothing
(script1.mlx) and the removal of isolated pieces, duplicate, zero-area and non-manifold faces (script2.mlx).
With --mesh-close-holes (implies --mesh) the small border loops of that mesh are filled on the GPU as script2.mlx's last filter, "Close
Holes", does: loops of at most N edges (30 when given bare) get their least-area triangulation, after --mesh-clean.
With --mesh-decimate (implies --mesh) that mesh is thinned to N faces (100000 when given bare) on the GPU as Demo/meshlab/decimation.mlx's
"Quadric Edge Collapse Decimation" does, after --mesh-close-holes and before the colouring.
With --mesh-subdivide (implies --mesh) that mesh is refined on the GPU as Demo/meshlab/subdiv.mlx's "Subdivision Surfaces: Loop" does: N
iterations (3 when given bare), each splitting every edge longer than --mesh-subdivide-threshold per cent of the mesh's box diagonal (1, the
script's value) -- after --mesh-decimate and before the colouring, whose resolution is the vertex density.  Limits: Loop's own
weights only (MeshLab's LoopWeight 0; the script's LoopWeight 2 is not built), vertex positions only, no colours carried across.
With --mesh-color (implies --mesh) the mesh's vertices are coloured from every camera's rectified image, on the GPU, where
CCloudOptimization::run calls TextureStitcher (visibility by a depth buffer per view, the best view or a cos-weighted blend; DESIGN.md 9
f9): the coloured mesh goes to the configuration's outfilename, where TextureStitcher's --out goes, and the cloud PLY to <name>_cloud.ply.
With --mesh-stitch (implies --mesh-color) the vertices take their best view's colour and the views' exposure seams are levelled on the
GPU by a screened gradient-domain solve on the mesh graph, TextureStitcher's seam removal; the same PLY at outfilename.
With --mesh-color-fill (implies --mesh-color) the vertices no view sees, grey after the colouring, are filled on the GPU with the harmonic
extension of the colours around them on the mesh graph, after --mesh-stitch when both are given: all of them that are
connected to a coloured vertex, or with ROUNDS those within that many edges of one; the same PLY at outfilename.
The rest of CCloudOptimization::run (main.cpp:19) is outside this package: feed bigcloud.ply or bigmesh.ply to it.
Needs an MI355X; there is no CPU path.
"""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np


class CloudSink:
    """Stands where CCloudOptimization stands in CStereoMatching::Init: collects what InsertPoint would receive."""

    def __init__(self):
        self.xyz, self.bgr = [], []

    def InsertPoints(self, xyz, bgr=None):   # one call per pair (the per-point InsertPoint order is preserved)
        self.xyz.append(np.asarray(xyz, np.float64))
        if bgr is not None:
            self.bgr.append(np.asarray(bgr, np.uint8))

    def filter(self, CamPair):               # no per-pair filter: the cloud as DisparityToCloud emits it
        pass


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m reconstruction_amd", description=__doc__.split("\n\n")[1])
    ap.add_argument("config", help="OpenCV-YAML configuration file (the reference's config_*.yml)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="PLY path (default: <outfilename of the configuration>.ply)")
    ap.add_argument("--radius", type=int, default=2, help="MatchBlockRadius (CReconstruction.cpp:17: 2)")
    ap.add_argument("--ws", type=float, default=0.03, help="smoothness weight (CReconstruction.cpp:17: 0.03)")
    ap.add_argument("--filter", action="store_true",
                    help="per-pair StatisticalOutlierRemoval (k=100, 1 sigma) as CCloudOptimization::filter (CReconstruction.cpp:18)")
    ap.add_argument("--outrem", nargs="*", default=None, metavar="N",
                    help="the filter (implied) with the RadiusOutlierRemoval of CCloudOptimization.cpp:90-96 behind its outlier removal: no value "
                         "(50 neighbours within radius 2, CReconstruction.cpp:18) or two, NEIGHBOURS RADIUS; give it after the configuration file")
    ap.add_argument("--mls-radius", type=float, default=2.5,
                    help="search radius of the per-pair normals and of the MLS, in scene units (m_mls_radius; CReconstruction.cpp:18 passes 2.5)")
    ap.add_argument("--mls", action="store_true",
                    help="after the filter (implied), CCloudOptimization::run's MLS over the merged cloud (order 1, normals flipped to the "
                         "filter's; CCloudOptimization.cpp:348-389) -> bigcloud.ply")
    ap.add_argument("--mls-out", default=None, help="path of the MLS cloud (default: bigcloud.ply next to the --out PLY)")
    ap.add_argument("--isdelete", action="store_true",
                    help="with --mls: the multi-view duplicate deletion before the MLS (Init's isdelete = true; CCloudOptimization.cpp:"
                         "152-346): one point per surface layer per pixel of the view each point faces best")
    ap.add_argument("--mesh", action="store_true",
                    help="after the MLS (implied): the surface of the smoothed cloud by unscreened Poisson reconstruction on a dense grid, "
                         "marching tetrahedra and a trim, on the GPU -> bigmesh.ply")
    ap.add_argument("--mesh-depth", type=int, default=9, help="2^depth grid nodes per axis: 5..9 on the dense grid (mesh.bat: --depth 9), 6..10 with --mesh-band (script1.mlx: OctDepth 10)")
    ap.add_argument("--mesh-trim", type=int, default=4,
                    help="faces survive within this many cells of a cell that holds a point (4 = mesh.bat's --trim 7 at depth 9; 0 = no trim)")
    ap.add_argument("--mesh-out", default=None, help="path of the mesh (default: bigmesh.ply next to the --out PLY)")
    ap.add_argument("--mesh-samples-per-node", type=float, nargs="?", const=2.0, default=None, metavar="S",
                    help="the surface (implied) with the density-adaptive splat: a sample is spread at the grid levels where a node would hold S of the "
                         "samples around it and weighs the inverse of their density (PoissonRecon --samplesPerNode; 2 when given bare as in mesh.bat, "
                         "script1.mlx: 3)")
    ap.add_argument("--mesh-band", type=int, nargs="?", const=1, default=None, metavar="B",
                    help="the surface (implied) one level finer than the dense grid reaches: --mesh-depth (6..10) is the finest depth, which exists only on "
                         "the bricks of 8^3 nodes within B (1..4; 1 when given bare) of a brick that holds a point, on top of the dense solve one depth "
                         "coarser; --mesh-trim is then at most 8 B - 1 (script1.mlx at depth 10 corresponds to --mesh-trim 8 --mesh-band 2); not with "
                         "--mesh-samples-per-node or --mesh-density-trim at depth 10")
    ap.add_argument("--mesh-band-samples-per-node", type=float, nargs="?", const=3.0, default=None, metavar="S",
                    help="the banded surface (--mesh-band 1 implied when that is absent) with the density-adaptive splat of --mesh-samples-per-node: the "
                         "levels below the finest are dense, the finest lives on the bricks (3 when given bare as in script1.mlx).  A switch of its own "
                         "because --mesh-band with --mesh-samples-per-node stays refused; honours --mesh-kernel-depth (0 or 3..depth - 1)")
    ap.add_argument("--mesh-kernel-depth", type=int, default=0, metavar="K",
                    help="with --mesh-samples-per-node or --mesh-band-samples-per-node: the density is estimated on 2^K grid nodes per axis, 3..depth "
                         "(on the band 3..depth - 1; 0 = depth - 2)")
    ap.add_argument("--mesh-density-trim", type=float, nargs="?", const=7.0, default=None, metavar="T",
                    help="after the surface (implied; --mesh-trim is then not applied): cut it where the smoothed sample-density value falls below T "
                         "(mesh.bat's SurfaceTrimmer --trim 7; 7 when given bare) on the GPU, before --mesh-clean")
    ap.add_argument("--mesh-density-smooth", type=int, default=100, help="with --mesh-density-trim: smoothing steps of the values (SurfaceTrimmer --smooth 100)")
    ap.add_argument("--mesh-island-ratio", type=float, default=0.01,
                    help="with --mesh-density-trim: pieces on either side of the cut below this share of the area change side (SurfaceTrimmer --aRatio 0.01; 0 = never)")
    ap.add_argument("--mesh-clean", action="store_true",
                    help="after the surface (implied): meshlab.bat's Laplacian smoothing and clean-up (isolated pieces, duplicate, zero-area "
                         "and non-manifold faces) on the GPU; bigmesh.ply is then the cleaned mesh")
    ap.add_argument("--mesh-smooth", type=int, default=5, help="with --mesh-clean: smoothing steps (script1.mlx: 5; 0 = none)")
    ap.add_argument("--mesh-min-piece", default="10%",
                    help="with --mesh-clean: pieces with a bounding-box diameter below this go; '10%%' = of the whole mesh's diagonal "
                         "(script2.mlx's ratio), a plain number = a length in scene units")
    ap.add_argument("--mesh-close-holes", type=int, nargs="?", const=30, default=None, metavar="N",
                    help="after the surface (implied; after --mesh-clean when given): fill every simple border loop of at most N edges (3..64; "
                         "script2.mlx's MaxHoleSize 30 when given bare) with its least-area triangulation on the GPU, before the mesh is written and coloured")
    ap.add_argument("--mesh-decimate", type=int, nargs="?", const=100000, default=None, metavar="N",
                    help="after the surface (implied; after --mesh-clean and --mesh-close-holes when given): thin the mesh to N faces (decimation.mlx's "
                         "TargetFaceNum 100000 when given bare) by quadric edge collapses on the GPU, before the mesh is written and coloured")
    ap.add_argument("--mesh-subdivide", type=int, nargs="?", const=3, default=None, metavar="N",
                    help="after the surface (implied; after --mesh-decimate when given): N iterations (1..8; subdiv.mlx's 3 when given bare) of Loop "
                         "subdivision on the GPU, before the mesh is written and coloured.  Loop's own weights only (MeshLab's LoopWeight 0; LoopWeight 1 "
                         "and 2, of which subdiv.mlx selects 2, are not built); positions only")
    ap.add_argument("--mesh-subdivide-threshold", type=float, default=1.0, metavar="PCT",
                    help="with --mesh-subdivide: only edges longer than PCT per cent of the mesh's box diagonal split (subdiv.mlx: 1; 0 = every edge)")
    ap.add_argument("--mesh-color", action="store_true",
                    help="after the surface (implied; after --mesh-clean when given): colour the mesh's vertices from the rectified views on the "
                         "GPU, where the reference calls TextureStitcher.  The coloured PLY goes to the configuration's outfilename (TextureStitcher's "
                         "--out), which is also --out's default: without --out the cloud PLY then goes to <name>_cloud.ply")
    ap.add_argument("--mesh-color-mode", choices=("best", "blend"), default="blend",
                    help="with --mesh-color: the colour of the best-facing visible view, or the cos-weighted blend of all visible views")
    ap.add_argument("--mesh-color-min-cos", type=float, default=0.2,
                    help="with --mesh-color: a view sees a vertex only at a cosine above this between its normal and the direction to the camera")
    ap.add_argument("--mesh-color-eps", type=float, default=None,
                    help="with --mesh-color: the depth test's slack in scene units (default: twice the Poisson grid step)")
    ap.add_argument("--mesh-stitch", action="store_true",
                    help="implies --mesh-color: level the views' exposure seams in the colours on the GPU (a screened gradient-domain solve on the "
                         "mesh graph).  It always colours by best view: --mesh-color-mode is not consulted.  The same PLY at outfilename")
    ap.add_argument("--mesh-stitch-lambda", type=float, default=0.01,
                    help="with --mesh-stitch: the pull towards the views' colours; a view's offset decays over about 1/sqrt(lambda) edges")
    ap.add_argument("--mesh-stitch-iterations", type=int, default=0,
                    help="with --mesh-stitch: Chebyshev steps (0: as many as reduce the error to 1e-4 of the start's)")
    ap.add_argument("--mesh-color-fill", type=int, nargs="?", const=0, default=None, metavar="ROUNDS",
                    help="implies --mesh-color (after --mesh-stitch when given): fill the vertices no view sees from the colours around them on the "
                         "GPU (the harmonic extension on the mesh graph): every one connected to a coloured vertex when given bare, else those within "
                         "ROUNDS edges of one.  The same PLY at outfilename")
    args = ap.parse_args(argv)
    outrem = None
    if args.outrem is not None:
        try:
            if len(args.outrem) not in (0, 2):
                raise ValueError("%d given" % len(args.outrem))
            outrem = (int(args.outrem[0]), float(args.outrem[1])) if args.outrem else (50, 2.0)
        except ValueError as e:
            print("--outrem takes no value or two, NEIGHBOURS (an integer) and RADIUS (a number): %s" % e)
            return 1
        args.filter = True
    if args.mesh_stitch or args.mesh_color_fill is not None:
        args.mesh_color = True
    if args.mesh_color:
        args.mesh = True
    if args.mesh_band_samples_per_node is not None and args.mesh_band is None:
        args.mesh_band = 1
    if args.mesh_density_trim is not None or args.mesh_close_holes is not None or args.mesh_decimate is not None or args.mesh_samples_per_node is not None or \
            args.mesh_subdivide is not None or args.mesh_band is not None:
        args.mesh = True
    if args.mesh_clean:
        args.mesh = True
        piece = args.mesh_min_piece.strip()
        try:
            min_piece, relative = (float(piece[:-1]) / 100.0, True) if piece.endswith("%") else (float(piece), False)
        except ValueError:
            ap.error("--mesh-min-piece: '%s' is neither a percentage like 10%% nor a length" % piece)
    if args.mesh:
        args.mls = True
    if args.isdelete and not args.mls:
        ap.error("--isdelete needs --mls (it selects the points the MLS reads)")
    if args.mls:
        args.filter = True

    from .config import load_config
    try:
        data, info = load_config(args.config)
    except (FileNotFoundError, ValueError) as e:
        print(e)                              # "cannot open file ..." (CReconstruction.cpp:9-13, CManageData.cpp:46-49)
        return 1
    from . import StereoMatching, write_ply   # loads the HIP library: fails loudly without it / without a GPU
    t0 = time.perf_counter()
    sm = StereoMatching(args.device)
    if args.filter:
        from . import CloudOptimization
        sink = CloudOptimization(sm._ctx)
        sink.Init(100, 1, outrem[0] if outrem else 50, outrem[1] if outrem else 2, args.mls_radius, data, args.isdelete)    # CReconstruction.cpp:18 (isdelete false there)
        if outrem:
            from . import RsmError
            try:
                sm._ctx.set_filter_outrem(*outrem)
            except RsmError as e:             # --outrem -1 2, --outrem 50 0: what rsm_filter_set_outrem refuses
                print(e)
                return 1
            sink.use_outrem = True
    else:
        sink = CloudSink()
    sm.Init(data, sink, args.radius, args.ws)
    sm.MatchAllLayer()
    print("Matching time: %.3f s" % (time.perf_counter() - t0))   # main.cpp:18
    if args.filter:
        if not sink.cloud_normals:
            print("no points")
            return 2
        xyz = np.concatenate([c[0] for c in sink.cloud_normals]).astype(np.float64)
        bgr = np.concatenate(sink.cloud_bgr)
        normals = np.concatenate([c[1] for c in sink.cloud_normals])
        if outrem:
            rep = [st["outrem"] for st in sink.stats]
            print("Radius outlier removal (more than %d within %g): %d points in, %d removed, %s"
                  % (outrem[0], outrem[1], sum(r["points_in"] for r in rep), sum(r["removed"] for r in rep),
                     "grid of radius-cells" if not any(r["window"] for r in rep) else "pixel window %d" % max(r["window"] for r in rep)))
    else:
        if not sink.xyz:
            print("no points")
            return 2
        xyz = np.concatenate(sink.xyz)
        bgr = np.concatenate(sink.bgr) if sink.bgr else np.zeros((len(xyz), 3), np.uint8)
    # the configuration's outfilename already carries its extension ("%s%d.ply", BatchProcess/main.cpp:56)
    name = data.outfilename or "cloud"
    out = args.out or (name if name.lower().endswith(".ply") else name + ".ply")
    color_out = None
    if args.mesh_color:                       # TextureStitcher's --out is the configuration's outfilename: the cloud steps aside
        color_out = name if name.lower().endswith(".ply") else name + ".ply"
        if args.out is None:
            out = color_out[:-4] + "_cloud.ply"
    write_ply(out, xyz, bgr, normals if args.filter else None)
    print("%d points -> %s" % (len(xyz), out))
    if args.mls:
        import os
        from . import write_ply_pointnormal
        t1 = time.perf_counter()
        try:
            mxyz, mnrm, _ = sink.run()
        except ValueError as e:                                    # --isdelete on pre-rectified input (no P)
            print(e)
            return 1
        if args.isdelete and sm.Verbose >= 1:
            st = sink.dedup_stats
            print("s1: %d s2: %d" % (st["s1"], st["s2"]))           # .cpp:194
            print("%d of %d points kept" % (len(sink.indicesptr), len(xyz)))
        big = args.mls_out or os.path.join(os.path.dirname(os.path.abspath(out)), "bigcloud.ply")
        write_ply_pointnormal(big, mxyz, mnrm)                     # savePLYFileBinary("tmp\\bigcloud.ply"), .cpp:389
        print("MLS time: %.3f s" % (time.perf_counter() - t1))
        print("%d points -> %s" % (len(mxyz), big))
    if args.mesh:
        from . import RsmError, write_ply_mesh
        t2 = time.perf_counter()
        try:
            mv, mf, mst = sink.mesh(depth=args.mesh_depth, trim_cells=args.mesh_trim if args.mesh_density_trim is None else 0,
                                    samples_per_node=args.mesh_samples_per_node, kernel_depth=args.mesh_kernel_depth, band_bricks=args.mesh_band,
                                    band_samples_per_node=args.mesh_band_samples_per_node)
        except (RsmError, ValueError) as e:                        # e.g. --mesh-depth outside 5..9, --mesh-samples-per-node 0, --mesh-band with it
            print(e)
            return 1
        cst = tst = hst = dst = ust = None
        if args.mesh_density_trim is not None:
            try:
                mv, mf, tst = sink.trim_mesh(smooth_steps=args.mesh_density_smooth, trim=args.mesh_density_trim, island_ratio=args.mesh_island_ratio)
            except RsmError as e:                                  # e.g. --mesh-island-ratio outside [0, 1)
                print(e)
                return 1
        if args.mesh_clean:
            try:
                mv, mf, cst = sink.clean_mesh(smooth_steps=args.mesh_smooth, min_piece=min_piece, relative=relative)
            except RsmError as e:                                  # e.g. a negative --mesh-smooth
                print(e)
                return 1
        if args.mesh_close_holes is not None:
            try:
                mv, mf, hst = sink.close_mesh_holes(max_hole_size=args.mesh_close_holes)
            except RsmError as e:                                  # --mesh-close-holes outside 3..64
                print(e)
                return 1
        if args.mesh_decimate is not None:
            try:
                mv, mf, dst = sink.decimate_mesh(target_faces=args.mesh_decimate)
            except RsmError as e:                                  # a negative --mesh-decimate
                print(e)
                return 1
        if args.mesh_subdivide is not None:
            try:
                mv, mf, ust = sink.subdivide_mesh(iterations=args.mesh_subdivide, threshold_fraction=args.mesh_subdivide_threshold / 100.0)
            except RsmError as e:                                  # --mesh-subdivide outside 1..8, a threshold outside 0..100
                print(e)
                return 1
        mesh_out = args.mesh_out or os.path.join(os.path.dirname(os.path.abspath(out)), "bigmesh.ply")
        write_ply_mesh(mesh_out, mv, mf)
        if args.mesh_band is not None:
            print("Mesh time: %.3f s (band of %d bricks around %d occupied; %d iterations from residual %.2e to %.2e on %d coarse cycles at %.2e%s)"
                  % (time.perf_counter() - t2, mst["active_bricks"], mst["occupied_bricks"], mst["iterations"], mst["residual_before"], mst["residual"],
                     mst["coarse_cycles"], mst["coarse_residual"], "" if mst["converged"] else ", NOT converged"))
        else:
            print("Mesh time: %.3f s (%d cycles, residual %.2e%s)" % (time.perf_counter() - t2, mst["cycles"], mst["residual"],
                                                                      "" if mst["converged"] else ", NOT converged"))
        spn = args.mesh_samples_per_node if args.mesh_band_samples_per_node is None else args.mesh_band_samples_per_node
        if spn is not None:
            print("Mesh samples per node %g: density on 2^%d nodes, %d of %d samples spread below depth %d (least depth %.2f)"
                  % (spn, mst["kernel_depth"], mst["n_below_depth"], mst["n_valid"], args.mesh_depth, mst["min_sample_depth"]))
        if tst is not None:
            print("Mesh density trim: %d faces from %d (%d split along %d cut edges); values %.2f .. %.2f; %d pieces moved to the kept side, %d to the dropped"
                  % (tst["n_faces"], tst["n_faces_in"], tst["faces_split"], tst["cut_edges"], tst["value_min"], tst["value_max"], tst["moved_to_kept"],
                     tst["moved_to_dropped"]))
        if cst is not None:
            print("Mesh clean: %d of %d pieces removed (%d faces); %d duplicate, %d zero-area, %d non-manifold faces removed; %d border vertices"
                  % (cst["components_removed"], cst["components"], cst["removed_isolated"], cst["removed_duplicate"], cst["removed_zero_area"],
                     cst["removed_nonmanifold"], cst["border_vertices"]))
        if hst is not None:
            print("Mesh close holes: %d of %d loops closed with %d faces (longest %d of %d); %d too long, %d lone triangles, %d without a triangulation; "
                  "%d open border components" % (hst["loops_closed"], hst["loops"], hst["faces_added"], hst["longest_closed"], hst["longest_loop"],
                                                 hst["loops_too_long"], hst["lone_triangles"], hst["loops_untriangulated"], hst["open_components"]))
        if dst is not None:
            print("Mesh decimate: %d -> %d faces (target %d%s) in %d rounds, %d collapses (%d of border edges); %d locked vertices, largest cost %.3g"
                  % (dst["n_faces_in"], dst["n_faces"], dst["target"], "" if dst["target_reached"] else ", not reached", dst["rounds"], dst["collapses"],
                     dst["border_collapses"], dst["locked_vertices"], dst["max_cost"]))
        if ust is not None:
            print("Mesh subdivide: %d -> %d faces, %d -> %d vertices in %d iterations (threshold %.6g); %d edges split (%d border, %d many-face); "
                  "faces with 0/1/2/3 splits %d/%d/%d/%d; %d interior and %d border vertices moved, %d locked"
                  % (ust["n_faces_in"], ust["n_faces"], ust["n_vertices_in"], ust["n_vertices"], ust["iterations"], ust["threshold"], ust["split_edges"],
                     ust["split_border_edges"], ust["split_many_face_edges"], ust["faces_0_splits"], ust["faces_1_split"], ust["faces_2_splits"],
                     ust["faces_3_splits"], ust["moved_interior"], ust["moved_border"], ust["locked_vertices"]))
        print("%d vertices, %d faces -> %s" % (len(mv), len(mf), mesh_out))
        if args.mesh_color:
            try:
                if args.mesh_stitch:
                    rgb, _, sst = sink.stitch_mesh(min_cos=args.mesh_color_min_cos, depth_eps=args.mesh_color_eps, lam=args.mesh_stitch_lambda,
                                                   iterations=args.mesh_stitch_iterations)
                else:
                    rgb, _, kst = sink.color_mesh(mode=1 if args.mesh_color_mode == "blend" else 0, min_cos=args.mesh_color_min_cos,
                                                  depth_eps=args.mesh_color_eps)
                if args.mesh_color_fill is not None:
                    rgb, _, fst = sink.fill_mesh_colors(max_rounds=args.mesh_color_fill)
            except (RsmError, ValueError) as e:                    # pre-rectified input (no P), --mesh-color-min-cos outside [-1, 1), a lambda <= 0, ROUNDS < 0
                print(e)
                return 1
            write_ply_mesh(color_out, mv, mf, rgb)
            if args.mesh_stitch:
                print("Mesh stitch: %d of %d vertices coloured from %d views, %d of %d incidences across a seam, %d steps (residual %.2e), largest "
                      "change %.2f levels -> %s" % (sst["coloured"], sst["n_vertices"], 2 * len(data.cam), sst["seam_incidences"], sst["incidences"],
                                                    sst["steps"], sst["rel_residual"], sst["max_change"], color_out))
            else:
                print("Mesh colour: %d of %d vertices coloured from %d views (%d without a normal) -> %s"
                      % (kst["coloured"], kst["n_vertices"], 2 * len(data.cam), kst["no_normal"], color_out))
            if args.mesh_color_fill is not None:
                print("Mesh colour fill: %d of %d uncoloured vertices filled in %d rounds, %d left as they were, %d steps, largest change from the "
                      "front's means %.2f levels -> %s" % (fst["filled"], fst["filled"] + fst["unreached"], fst["rounds"], fst["unreached"], fst["steps"],
                                                           fst["max_change"], color_out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
