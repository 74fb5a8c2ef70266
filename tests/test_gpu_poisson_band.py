"""The banded finest level of the GPU Poisson surface (csrc/k_poisson_band.hip) against its numpy restatement
(tests/poisson_band_restatement.py, held to the dense restatement and to exact solves without a GPU in tests/test_poisson_band_cpu.py):
the bricks, the occupancy and the guess to the bit and the right-hand side within f7's fixed-point bound; the band solve's residual
iteration by iteration; the extraction and the trim byte for byte on constructed fields over a brick pattern with holes; the whole call on
the sphere; the refusals; the API / CLI switch.  The largest grid is 128^3 (the right-hand side of the sparse fixture); no test needs depth 10.

Figures (MI355X; 21 tests in 7.4 s):
  rhs stage        bricks, occ and g equal on every input; max |b - restatement| 1.0e-9 where the bound is 4.3e-9; sparse fixture 432 of 4096 bricks
  history          the GPU's residuals equal the restatement's float32 ones to 2e-16; float32 against fp64 7.2e-3 (225 of 512 bricks, 34 iterations
                   compared) and 1.3e-2 (512 of 512, 40): tol 7.2e-2 and 1.3e-1
  all active       48 iterations (restatement 48) to 3.740e-5, true residual 3.738e-5; max |chi - exact| / range 1.975e-4 (restatement 1.975e-4)
  extraction       269 bricks: 395 090 vertices, 714 200 faces (random), 686 132 (tie0), 682 800 (tie1); least whole-cell case count 4 906;
                   trims of 1, 3, 7 cells keep 1 599, 12 345, 63 397 faces
  whole call       sphere, depth 6: 47 560 vertices, 95 116 faces (the dense restatement's counts), 504 of 512 bricks, coarse 10 cycles, band 41
                   iterations 8.672e-1 -> 3.550e-5, max radial error 0.27207 h (dense restatement 0.27212 h)
  rig              run() -> mesh(depth=7, band_bricks=1): 13 296 faces (dense depth 6: 5 316), 444 bricks, 31 iterations"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import poisson_band_restatement as pb
import poisson_restatement as pr
from reconstruction_amd import RsmError, _lib, synth
from reconstruction_amd._mesh import POISSON_REL_RESIDUAL

pytestmark = pytest.mark.gpu

CLOSED = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0, edge_without_opposite=0, edges_not_in_two_faces=0, unused_vertices=0, euler=2)
_cache = {}


def same_bits(a, b):
    """(a call, so that a failure shows False and not a diff of two long byte strings)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def corner_samples():
    """two samples, each in a corner cell of the grid they span (scale 1: they lie on the box's corners and their cells are clamped)"""
    return pr._with_normals(np.array([[-3.0, 2.0, 10.0], [5.0, 10.0, 18.0]]), np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]]))


# name -> (samples, depth, scale, band_bricks)
INPUTS = {"sphere": (lambda: pr.sphere_samples(80000), 6, 1.1, 1), "sparse": (lambda: pb.sparse_fixture()[0], 7, 3.0, 1),
          "two_spheres": (lambda: pr.two_spheres_samples(60000), 7, 1.1, 1), "plate": (lambda: pr.plate_samples(20000), 6, 1.0, 1),
          "corners": (corner_samples, 6, 1.0, 2)}


def rhs_ref(name):
    def make():
        make_samples, depth, scale, band = INPUTS[name]
        xyz, nrm = make_samples()
        R = pb.band_rhs(xyz, nrm, depth, scale, band)
        R.update(xyz=xyz, nrm=nrm, depth=depth, scale=scale, band=band)
        R["chi_c"] = np.random.default_rng(31).normal(size=((1 << depth) >> 1,) * 3).astype(np.float32)    # any coarse field: the guess is its prolongation
        return R
    return cached(("rhs", name), make)


# ---- 1: bricks, splat, right-hand side, guess ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(INPUTS))
def test_rhs_stage_against_the_restatement(ctx, name):
    R = rhs_ref(name)
    G = ctx.poisson_band_rhs(R["xyz"], R["nrm"], R["depth"], R["scale"], R["band"], chi_c=R["chi_c"])
    B = R["active"].shape[0]
    print("%s: depth %d, %d of %d bricks active, %d occupied" % (name, R["depth"], len(R["bricks"]), B ** 3, int(R["occupied"].sum())))
    assert np.array_equal(G["bricks"], R["bricks"]) and G["bricks"].dtype == np.int32
    assert G["counts"] == (len(R["p"]), R["n_invalid"], len(R["bricks"]), int(R["occupied"].sum()))
    assert np.array_equal(G["grid"][:3], R["o"]) and G["grid"][3] == R["h"]
    assert same_bits(G["occ"], pb.to_bricks(R["occ"], R["bricks"]))
    assert same_bits(G["g"], pb.to_bricks(pb.guess(R["chi_c"]), R["bricks"]))
    bound = pb.to_bricks(pr.rhs_fixed_point_bound(R["cnt"], R["b"]), R["bricks"])
    dev = np.abs(G["b"] - pb.to_bricks(R["b"], R["bricks"]))
    print("  max |b - restatement| %.3e (bound there %.3e)" % (dev.max(), bound.ravel()[dev.argmax()]))
    assert (dev <= bound).all() and np.abs(G["b"]).max() > 0
    if name == "two_spheres":                                                                # two pieces: no brick holds samples of both
        which = np.abs(np.linalg.norm(R["p"][:, None, :] - pr.TWO_C[None], axis=2) - pr.TWO_R).argmin(1)
        cell = np.clip(np.floor((R["p"] - R["o"]) / R["h"]).astype(np.int64), 0, 8 * B - 1) >> 3
        lin = cell[:, 0] + B * (cell[:, 1] + B * cell[:, 2])
        assert len(set(lin[which == 0].tolist())) > 50 and len(set(lin[which == 1].tolist())) > 10 and not set(lin[which == 0].tolist()) & set(lin[which == 1].tolist())
    if name == "plate":                                                                      # bricks on the grid's faces: neighbour lookups leave the grid
        bx = R["bricks"] % B
        assert (bx == 0).any() and (bx == B - 1).any()
    if name == "corners":
        assert {0, B ** 3 - 1} <= set(R["bricks"].tolist()) and int(R["occupied"].sum()) == 2 and len(R["bricks"]) == 54
    if name == "sparse":
        assert len(R["bricks"]) <= 0.15 * B ** 3


def test_rhs_stage_with_its_own_coarse_solve_and_nothing_to_mesh(ctx):
    R = rhs_ref("sphere")
    G = ctx.poisson_band_rhs(R["xyz"], R["nrm"], 6)                                         # the guess from the library's dense solve at depth 5
    chi_c = ctx.poisson_solve(ctx.poisson_rhs(R["xyz"], R["nrm"], 5)[1])[0]
    assert G["status"] == 0 and same_bits(G["g"], pb.to_bricks(pb.guess(chi_c), R["bricks"]))
    one = pr._with_normals(np.array([[1.0, 2.0, 3.0]]), np.array([[0.0, 0.0, 1.0]]))       # a single sample: side = 0
    for xyz, nrm, valid in (one + (1,), (np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), 0)):
        E = ctx.poisson_band_rhs(xyz, nrm, 6)
        assert E["grid"][3] == 0.0 and E["counts"] == (valid, 0, 0, 0) and len(E["bricks"]) == 0
        v, f, st = ctx.poisson_mesh_banded(xyz, nrm, 6)
        assert v.shape == (0, 3) and f.shape == (0, 3) and st["status"] == 0 and st["n_valid"] == valid and st["active_bricks"] == 0


# ---- 2: the band solve -------------------------------------------------------------------------------------------------------------------
SOLVES = {"half": (6, 80000, 2.0, 1), "full": (6, 80000, 1.1, 2)}                            # depth, samples of the sphere, scale, band_bricks
ITERATIONS = 40


def solve_ref(name):
    """the band right-hand side and guess as the library reads them (float32), the restatement's histories in both precisions"""
    def make():
        depth, n, scale, band = SOLVES[name]
        xyz, nrm = pr.sphere_samples(n)
        R = pb.band_rhs(xyz, nrm, depth, scale, band)
        Vc, _, _ = pr.splat(R["p"], R["nh"], R["o"], 2.0 * R["h"], depth - 1)
        R["chi_c"] = pr.solve_exact(pr.rhs(Vc)).astype(np.float32)
        R["g"] = pb.guess(R["chi_c"])
        R["b32"] = R["b"].astype(np.float32)
        R["r64"], R["h64"], _ = pb.band_pcg(R["b32"].astype(np.float64), R["g"].astype(np.float64), R["mask"], ITERATIONS, np.float64)
        R["r32"], R["h32"], _ = pb.band_pcg(R["b32"], R["g"], R["mask"], ITERATIONS, np.float32)
        R["depth"] = depth
        return R
    return cached(("solve", name), make)


@pytest.mark.parametrize("name", list(SOLVES))
def test_history_follows_the_restatement_iteration_by_iteration(ctx, name):
    """As for f7's solver (test_gpu_poisson_stages.py): conjugate gradients converge with any symmetric positive preconditioner, so a wrong
    neighbour slot, colour or boundary term costs iterations and shows in the residual after every iteration, not in `converged`.  tol is the
    restatement's own float32 against fp64 history over the compared iterations times 10, at least 1e-3; iterations below 1e-4 are left out."""
    R = solve_ref(name)
    bricks = R["bricks"]
    chi, res, its, status, hist, res0 = ctx.poisson_band_solve(bricks, R["depth"], pb.to_bricks(R["b32"], bricks), pb.to_bricks(R["g"], bricks), R["chi_c"],
                                                               rel_residual=1e-12, max_iterations=ITERATIONS)
    h64, h32 = R["h64"], R["h32"]
    sel = np.nonzero(h64 >= 1e-4)[0]
    assert len(h64) == ITERATIONS and len(sel) >= 20 and len(hist) > sel.max()
    tol = max(1e-3, 10.0 * np.abs(h32[sel] / h64[sel] - 1.0).max())
    fmt = lambda h: " ".join("%.3e" % x for x in h)
    print("%s: %d of %d bricks\n  GPU     %.4e | %s\n  float32 %.4e | %s\n  fp64    %.4e | %s" % (name, len(bricks), R["active"].size, res0, fmt(hist), R["r32"], fmt(h32),
                                                                                                      R["r64"], fmt(h64)))
    dev = np.abs(hist[sel] / h64[sel] - 1.0)
    print("  iterations compared %d, tol %.3e, max |GPU / fp64 - 1| %.3e, against float32 %.3e" % (len(sel), tol, dev.max(), np.abs(hist[sel] / h32[sel] - 1.0).max()))
    assert abs(res0 / R["r64"] - 1.0) <= 1e-3 and (dev <= tol).all()
    assert status == 1 and res == hist.min()


def test_all_bricks_active_against_the_direct_solution(ctx):
    R = solve_ref("full")
    bricks = R["bricks"]
    assert len(bricks) == 512
    exact = pr.solve_exact(R["b32"].astype(np.float64))
    rng_ = exact.max() - exact.min()
    S = pb.band_solve(R["b32"], R["g"], R["mask"], POISSON_REL_RESIDUAL, 200)
    gap = np.abs(S["chi"].astype(np.float64) - exact).max() / rng_
    chi, res, its, status, hist, res0 = ctx.poisson_band_solve(bricks, 6, pb.to_bricks(R["b32"], bricks), pb.to_bricks(R["g"], bricks))   # no coarse field: nothing is off the band
    dense = pb.from_bricks(chi, bricks, 6).astype(np.float64)
    fig = np.abs(dense - exact).max() / rng_
    true = np.linalg.norm(R["b32"] - pr.apply_L(dense)) / np.linalg.norm(R["b32"])
    print("all active: GPU %d iterations (restatement %d) to %.3e, true residual %.3e; max |chi - exact| / range %.3e (restatement %.3e)" %
          (its, S["iterations"], res, true, fig, gap))
    assert status == 0 and res <= POISSON_REL_RESIDUAL and abs(its - S["iterations"]) <= 1
    assert abs(true - res) <= 0.05 * POISSON_REL_RESIDUAL
    assert fig <= 4.0 * gap


def test_solve_keeps_the_best_iterate_and_repeats(ctx):
    R = solve_ref("half")
    bricks = R["bricks"]
    args = (bricks, 6, pb.to_bricks(R["b32"], bricks), pb.to_bricks(R["g"], bricks), R["chi_c"])
    a = ctx.poisson_band_solve(*args)
    b = ctx.poisson_band_solve(*args)
    assert same_bits(a[0], b[0]) and a[1:4] == b[1:4] and np.array_equal(a[4], b[4]) and a[3] == 0 and a[1] <= POISSON_REL_RESIDUAL
    one = ctx.poisson_band_solve(*args, max_iterations=1)
    assert one[2] == 1 and one[3] == 1 and one[1] == min(one[5], one[4][0]) == a[4][0] and one[5] == a[5]
    floor = ctx.poisson_band_solve(*args, rel_residual=1e-12, max_iterations=200)            # below the float32 floor: ends STALL iterations after its best
    assert floor[3] == 1 and floor[2] < 200 and floor[1] == floor[4].min() and int(np.argmin(floor[4])) + 1 == floor[2] - pb.STALL
    cut = ctx.poisson_band_solve(*args, rel_residual=1e-12, max_iterations=floor[2] - pb.STALL)
    assert same_bits(cut[0], floor[0])
    z = ctx.poisson_band_solve(bricks, 6, np.zeros((len(bricks), 512), np.float32), args[3], R["chi_c"])
    assert z[1] == 0.0 and z[2] == 0 and z[3] == 0 and same_bits(z[0], args[3])                # b = 0: the guess comes back


# ---- 3: extraction and trim on constructed fields --------------------------------------------------------------------------------------------
def holes():
    bricks = pb.holes_pattern(6)
    return bricks, pb.node_mask(pb.active_of_list(bricks, 6))


@pytest.mark.parametrize("kind", ["random", "tie0", "tie1"])
def test_extraction_of_constructed_fields_equals_the_restatement(ctx, kind):
    """A checkerboard of bricks plus a solid 3 x 3 x 3 block: every kind of neighbour (face, edge, corner; active, inactive, outside the grid)
    occurs, and a cell with an inactive corner must give no face.  'random': all 14 mixed cases of all six tetrahedra occur in whole cells;
    'tie0' / 'tie1': integer values with iso among them (t = 0, coincident vertices)."""
    bricks, mask = holes()
    chi, iso = pr.lattice_field(kind, 64)
    v, f, keys, _ = cached(("extract", kind), lambda: pb.extract_band(chi, iso, pr.FIELD_O, pr.FIELD_H, bricks))
    grid = np.concatenate([pr.FIELD_O, [pr.FIELD_H]])
    gv, gf = ctx.band_iso_mesh(bricks, 6, pb.to_bricks(chi, bricks), iso, grid)
    counts = pb.tet_case_counts_band(chi, iso, mask)
    print("%s: %d bricks, %d vertices, %d faces; least whole-cell case count %d" % (kind, len(bricks), len(v), len(f), counts[:, 1:15].min()))
    assert len(f) > 100000 and same_bits(gv, v) and same_bits(gf, f)
    if kind == "random":
        assert (counts[:, 1:15] > 0).all()


def test_trim_and_empty_extractions(ctx):
    bricks, mask = holes()
    chi, iso = pr.lattice_field("random", 64)
    grid = np.concatenate([pr.FIELD_O, [pr.FIELD_H]])
    v, f, keys, _ = cached(("extract", "random"), lambda: pb.extract_band(chi, iso, pr.FIELD_O, pr.FIELD_H, bricks))
    occ = np.zeros((64, 64, 64), np.uint8)                                                  # cells of the block's middle brick: a dilation by <= 7 stays in the block
    occ[8:16, 8:16, 8:16] = np.random.default_rng(5).uniform(size=(8, 8, 8)) < 0.02
    assert occ.sum() >= 4
    for trim_cells in (1, 3, 7):
        tv, tf = pb.trim_band(v, f, occ, pr.FIELD_O, pr.FIELD_H, trim_cells, 1)
        gv, gf = ctx.band_iso_mesh(bricks, 6, pb.to_bricks(chi, bricks), iso, grid, pb.to_bricks(occ, bricks), trim_cells)
        print("trim %d: %d of %d faces" % (trim_cells, len(tf), len(f)))
        assert 0 < len(tf) < len(f) and same_bits(gv, tv) and same_bits(gf, tf)
    for field, level in ((np.full((64, 64, 64), 1.0, np.float32), 0.5), (chi, 100.0)):       # nothing crosses
        gv, gf = ctx.band_iso_mesh(bricks, 6, pb.to_bricks(field, bricks), level, grid)
        assert gv.shape == (0, 3) and gf.shape == (0, 3)
    gv, gf = ctx.band_iso_mesh(np.zeros(0, np.int32), 6, np.zeros((0, 512), np.float32), 0.0, grid)
    assert gv.shape == (0, 3) and gf.shape == (0, 3)
    one = np.array([73], np.int32)                                                          # a lone brick: 7^3 whole cells
    lv, lf, _, _ = pb.extract_band(chi, iso, pr.FIELD_O, pr.FIELD_H, one)
    gv, gf = ctx.band_iso_mesh(one, 6, pb.to_bricks(chi, one), iso, grid)
    assert len(lf) > 100 and same_bits(gv, lv) and same_bits(gf, lf)


# ---- 4: the whole call -----------------------------------------------------------------------------------------------------------------------
def sphere_call(ctx):
    def make():
        xyz, nrm = pr.sphere_samples(80000)
        return xyz, nrm, ctx.poisson_mesh_banded(xyz, nrm, 6, trim_cells=4)
    return cached("sphere_call", make)


def test_whole_call_on_the_sphere(ctx):
    """The sphere's maximum radial error within 0.005 h of the dense restatement's at the same depth (the restatements differ by <= 1e-4 h, f7's
    GPU call from its restatement by 2e-4 h: 0.005 h covers the float32 solve and nothing coarser); closed and manifold after the trim."""
    xyz, nrm, (v, f, st) = sphere_call(ctx)
    def dense():                                                                             # f7's restatement with the direct solution of its system
        Q = pr.rhs_of(xyz, nrm, 6)
        chi = pr.solve_exact(Q["b"])
        v0, f0, _ = pr.extract(chi.astype(np.float32), pr.iso_value(chi, Q["p"], Q["o"], Q["h"]), Q["o"], Q["h"])
        tv, tf = pr.trim(v0, f0, Q["occ"], Q["o"], Q["h"], 4)
        return dict(verts=tv, faces=tf, h=Q["h"])
    D = cached("dense6", dense)
    R = rhs_ref("sphere")
    err, derr = pr.radial_error_h(v, st["h"]).max(), pr.radial_error_h(D["verts"], D["h"]).max()
    print("sphere depth 6: %d vertices, %d faces (dense restatement %d, %d); %d of 512 bricks; coarse %d cycles to %.2e; band %d iterations %.3e -> %.3e; "
          "max radial error %.5f h (dense restatement %.5f h)" % (len(v), len(f), len(D["verts"]), len(D["faces"]), st["active_bricks"], st["coarse_cycles"],
                                                                  st["coarse_residual"], st["iterations"], st["residual_before"], st["residual"], err, derr))
    assert st["status"] == 0 and st["converged"] and st["residual"] <= POISSON_REL_RESIDUAL < st["residual_before"] and st["coarse_residual"] <= POISSON_REL_RESIDUAL
    assert st["N"] == 64 and st["h"] == R["h"] and st["origin"] == tuple(R["o"]) and st["n_valid"] == 80000 and st["n_invalid"] == 0
    assert st["active_bricks"] == len(R["bricks"]) and st["occupied_bricks"] == int(R["occupied"].sum())
    assert abs(err - derr) <= 0.005
    assert pr.manifold_report(v, f) == CLOSED and pr.face_orientation_min(v, f) > 0.0
    assert st["n_faces_untrimmed"] >= len(f) > 10000


def test_two_calls_and_both_entries_return_the_same_bytes(ctx):
    xyz, nrm, (v1, f1, s1) = sphere_call(ctx)
    v2, f2, s2 = ctx.poisson_mesh_banded(xyz, nrm, 6, trim_cells=4)
    assert same_bits(v1, v2) and same_bits(f1, f2) and s1 == s2 and len(f1) > 1000
    dx, dn = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
    nv, nf, s3 = ctx.poisson_mesh_banded_device(dx.data_ptr(), dn.data_ptr(), len(xyz), 6, trim_cells=4)
    assert (nv, nf) == (len(v1), len(f1)) and s3 == s1
    dv = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    df = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    ctx.poisson_last_mesh_device(dv.data_ptr(), df.data_ptr())
    torch.cuda.synchronize()
    assert dv.cpu().numpy().tobytes() == v1.tobytes() and df.cpu().numpy().tobytes() == f1.tobytes()
    r1, r2 = ctx.poisson_band_rhs(xyz, nrm, 6), ctx.poisson_band_rhs(xyz, nrm, 6)
    assert all(same_bits(np.asarray(r1[k]), np.asarray(r2[k])) for k in ("grid", "bricks", "b", "occ", "g"))


def test_invalid_samples_not_converged_and_no_trim(ctx):
    xyz, nrm, (v, f, st) = sphere_call(ctx)
    bad_x = np.array([[np.nan, 0, 0], [1, 2, 3], [np.inf, 0, 0], [5, 5, 5]], np.float32)
    bad_n = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0], [np.nan, 0, 0, 0]], np.float32)
    mx, mn = np.concatenate([bad_x[:2], xyz, bad_x[2:]]), np.concatenate([bad_n[:2], nrm, bad_n[2:]])
    v2, f2, st2 = ctx.poisson_mesh_banded(mx, mn, 6, trim_cells=4)
    assert same_bits(v2, v) and same_bits(f2, f) and st2["n_invalid"] == 4 and st2["n_valid"] == 80000
    v1, f1, st1 = ctx.poisson_mesh_banded(xyz, nrm, 6, trim_cells=4, max_iterations=1)        # RSM_W_NOT_CONVERGED: the mesh of the best field
    assert st1["status"] == _lib.RSM_W_NOT_CONVERGED and not st1["converged"] and st1["iterations"] == 1 and st1["residual"] > POISSON_REL_RESIDUAL
    assert len(f1) > 1000 and f1.min() >= 0 and f1.max() < len(v1) and np.isfinite(v1).all() and pr.manifold_report(v1, f1)["index_out_of_range"] == 0
    vc, fc, stc = ctx.poisson_mesh_banded(xyz, nrm, 6, trim_cells=4, max_cycles=1)            # ... also when the coarse solve ended early
    assert stc["status"] == _lib.RSM_W_NOT_CONVERGED and stc["coarse_cycles"] == 1 and stc["coarse_residual"] > POISSON_REL_RESIDUAL and len(fc) > 1000
    v0, f0, st0 = ctx.poisson_mesh_banded(xyz, nrm, 6, scale=2.0, trim_cells=0)                # no trim: the sphere never leaves its band
    rep = pr.manifold_report(v0, f0)
    assert st0["active_bricks"] < 400 and rep["edges_not_in_two_faces"] == 0 and rep["index_out_of_range"] == 0 and (len(v0), len(f0)) == (st0["n_vertices_untrimmed"], st0["n_faces_untrimmed"])
    pv, pf, pst = ctx.poisson_mesh_banded(*pr.plate_samples(20000), 6, scale=1.0, trim_cells=0)  # ... an open surface does: borders where the band ends
    rep = pr.manifold_report(pv, pf)
    assert len(pf) > 1000 and rep["edges_not_in_two_faces"] > 0 and rep["index_out_of_range"] == 0 and rep["directed_edge_twice"] == 0
    v7, f7, st7 = ctx.poisson_mesh_banded(xyz, nrm, 6, scale=2.0, trim_cells=7)                # the widest trim of band_bricks 1
    assert pr.manifold_report(v7, f7) == CLOSED


def test_invalid_parameters_are_named(ctx):
    xyz, nrm = pr.sphere_samples(2000)
    dx, dn = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
    cases = ((dict(depth=5), "depth"), (dict(depth=11), "depth"), (dict(band_bricks=0), "band_bricks"), (dict(band_bricks=5), "band_bricks"),
             (dict(max_iterations=0), "max_iterations"), (dict(trim_cells=8), "trim_cells"), (dict(trim_cells=16, band_bricks=2), "trim_cells"),
             (dict(trim_cells=-1), "trim_cells"), (dict(scale=0.5), "scale"), (dict(rel_residual=0.0), "rel_residual"), (dict(max_cycles=0), "max_cycles"))
    for kw, word in cases:
        with pytest.raises(RsmError, match=word):
            ctx.poisson_mesh_banded(xyz, nrm, **{**dict(depth=6), **kw})
        with pytest.raises(RsmError, match=word):
            ctx.poisson_mesh_banded_device(dx.data_ptr(), dn.data_ptr(), len(xyz), **{**dict(depth=6), **kw})
    v, f, st = ctx.poisson_mesh_banded(xyz, nrm, 6, trim_cells=15, band_bricks=2)              # 8 band_bricks - 1 is allowed
    assert st["status"] in (0, 1)
    with pytest.raises(RsmError, match=r"\b%d active bricks" % len(pb.band_rhs(xyz, nrm, 6)["bricks"])):   # the cap, lowered through the stage's argument
        ctx.poisson_band_rhs(xyz, nrm, 6, max_bricks=10)
    with pytest.raises(RsmError, match="max_bricks"):
        ctx.poisson_band_rhs(xyz, nrm, 6, max_bricks=(1 << 20) + 1)
    bricks = np.array([3, 9, 100], np.int32)
    z = np.zeros((3, 512), np.float32)
    grid = np.array([0.0, 0.0, 0.0, 1.0])
    for bad, word in ((np.array([3, 3, 100], np.int32), r"bricks\[1\]"), (np.array([3, 100, 9], np.int32), r"bricks\[2\]"), (np.array([3, 9, 512], np.int32), r"bricks\[2\]"),
                      (np.array([-1, 9, 100], np.int32), r"bricks\[0\]")):
        with pytest.raises(RsmError, match=word):
            ctx.band_iso_mesh(bad, 6, z, 0.0, grid)
        with pytest.raises(RsmError, match=word):
            ctx.poisson_band_solve(bad, 6, z, z)
    for kw, word in ((dict(depth=5), "depth"), (dict(depth=11), "depth")):
        with pytest.raises(RsmError, match=word):
            ctx.band_iso_mesh(bricks, kw["depth"], z, 0.0, grid)
    with pytest.raises(RsmError, match="trim_cells"):
        ctx.band_iso_mesh(bricks, 6, z, 0.0, grid, trim_cells=-1)
    with pytest.raises(RsmError, match="grid"):
        ctx.band_iso_mesh(bricks, 6, z, 0.0, np.array([0.0, 0.0, 0.0, 0.0]))
    with pytest.raises(RsmError, match="max_iterations"):
        ctx.poisson_band_solve(bricks, 6, z, z, max_iterations=0)
    with pytest.raises(RsmError, match="rel_residual"):
        ctx.poisson_band_solve(bricks, 6, z, z, rel_residual=1.0)
    prm, bpr = _lib.PoissonParams(6, 1.1, 0.5, 1, 0), _lib.PoissonBandParams(1, 1)
    nv, nf = C.c_int64(), C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = ctx._lib
    assert lib.rsm_poisson_mesh_banded(ctx._h, p(xyz), p(nrm), 2000, C.byref(prm), None, C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_poisson_mesh_banded(ctx._h, p(xyz), p(nrm), 2000, None, C.byref(bpr), C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_poisson_mesh_banded(ctx._h, None, p(nrm), 2000, C.byref(prm), C.byref(bpr), C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_poisson_mesh_banded_device(ctx._h, None, None, 2000, C.byref(prm), C.byref(bpr), C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_poisson_mesh_banded(ctx._h, p(xyz), p(nrm), -1, C.byref(prm), C.byref(bpr), C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    with pytest.raises(RsmError, match="depth"):                                             # the dense call keeps its range
        ctx.poisson_mesh(xyz, nrm, 10)


# ---- 5: the later stages, the API and the CLI ------------------------------------------------------------------------------------------------
def test_chain_banded_mesh_then_clean(ctx):
    xyz, nrm = pr.sphere_samples(80000)
    v, f, st = ctx.poisson_mesh_banded(xyz, nrm, 6, trim_cells=4)
    cv, cf, cst = ctx.mesh_clean_last()
    assert cst["n_vertices_in"] == len(v) and cst["n_faces_in"] == len(f) and 0 < len(cf) <= len(f) and cst["components"] == 1
    ev, ef, est = ctx.mesh_clean(v, f)
    assert same_bits(cv, ev) and same_bits(cf, ef)


def test_cloud_optimization_mesh_with_band_bricks(ctx):
    from reconstruction_amd import Camera, CloudOptimization, ManageData, StereoMatching
    cfgs = [synth.config_small(320, 192, 3, radius=2, pair=4, mask_l0_width=60, border_l0=4),
            synth.config_small(320, 192, 3, radius=2, pair=5, mask_l0_width=50, border_l0=4, holes=True)]
    cam = np.array([0.0, 0.0, 0.0], np.float32)
    top = 1 << (cfgs[0].pyr_levels - 1)
    data = ManageData(cam=[[Camera(camID=0, image=c.image[0], mask=c.mask[0], CamCenter=cam),
                            Camera(camID=1, image=c.image[1], mask=c.mask[1], CamCenter=cam)] for c in cfgs],
                      m_PyrmNum=cfgs[0].pyr_levels, m_LowestLevelSize=(cfgs[0].width // top, cfgs[0].height // top),
                      m_OriginSize=(cfgs[0].width, cfgs[0].height),
                      rectified=[dict(Q=c.Q, R_final=c.R_final, T_final=c.T_final) for c in cfgs])
    opt = CloudOptimization(ctx)
    opt.Init(100, 1, 50, 2, 40.0, data, False)
    sm = StereoMatching(0)
    sm.Init(data, opt, 2, 0.03)
    sm.Verbose = 0
    sm.MatchAllLayer()
    sx, sn, _ = opt.run()
    pv, pf, pst = opt.mesh(depth=6)
    ev, ef, est = ctx.poisson_mesh(sx, sn, 6)
    assert same_bits(pv, ev) and same_bits(pf, ef) and pst == est and "active_bricks" not in pst               # None is the dense call
    v, f, st = opt.mesh(depth=7, band_bricks=1)
    assert opt.mesh_result[0] is v and opt.mesh_grid_step == st["h"] and st["N"] == 128
    bv, bf, bst = ctx.poisson_mesh_banded(sx, sn, 7, trim_cells=4, band_bricks=1)
    print("run() -> mesh(depth=7, band_bricks=1): %d faces (dense depth 6: %d); %d bricks, %d iterations" % (len(f), len(pf), st["active_bricks"], st["iterations"]))
    assert same_bits(v, bv) and same_bits(f, bf) and st == bst and len(f) > len(pf) > 1000
    with pytest.raises(ValueError, match="samples_per_node"):
        opt.mesh(depth=7, band_bricks=1, samples_per_node=2)
    cv, cf, cst = opt.clean_mesh()                                                                          # the later stages run on the result
    assert cst["n_faces_in"] == len(f) and 0 < len(cf) <= len(f)


def test_cli_mesh_band(ctx, tmp_path, capsys):
    from PIL import Image
    from reconstruction_amd import config as cfgmod
    from reconstruction_amd.__main__ import main
    raw = synth.make_raw_pair(baseline=-150.0)
    root = str(tmp_path) + "/"
    (tmp_path / "mask").mkdir()
    for j in range(2):
        Image.fromarray(raw["image"][j][:, :, ::-1]).save(root + "0001_Cam%d.png" % j)
        Image.fromarray(raw["mask"][j]).save(root + "mask/0001_Cam%d.png" % j)
    cfgmod.dump_opencv_yaml(root + "calib_camera.yml", {"intrinsic-0": raw["K"][0], "extrinsic-0": raw["E"][0],
                                                         "intrinsic-1": raw["K"][1], "extrinsic-1": raw["E"][1]})
    cfgmod.dump_opencv_yaml(root + "config.yml", {
        "filepath": root, "outfilename": root + "out", "isoutput": 0, "camera_calib_name": "calib_camera.yml",
        "PyrmNum": raw["pyr_levels"], "LowestLevelWidth": raw["lowest"][0], "LowestLevelHeight": raw["lowest"][1],
        "imagelist": ["0001_Cam%d.png" % j for j in range(2)], "masklist": ["mask\\0001_Cam%d.png" % j for j in range(2)],
        "camID": np.array([[0, 1]], np.uint8)})
    norm = lambda s: re.sub(r"\d+\.\d+ s", "T s", s)
    base = [root + "config.yml", "--mls-radius", "10", "--mesh-depth", "7"]
    capsys.readouterr()
    assert main(base + ["--mesh-band"]) == 0                                                                # bare: 1; implies --mesh
    out = norm(capsys.readouterr().out)
    v, f = pr.read_ply_mesh(root + "bigmesh.ply")
    blob = open(root + "bigcloud.ply", "rb").read()
    rec = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], "<f4").reshape(-1, 7)
    sx, sn = rec[:, :3].copy(), rec[:, 3:].copy()
    ev, ef, est = ctx.poisson_mesh_banded(sx, sn, 7, trim_cells=4, band_bricks=1)
    assert same_bits(v, ev) and np.array_equal(f, ef) and len(f) > 1000
    lines = out.splitlines()
    assert lines[-2].startswith("Mesh time: T s (band of %d bricks around %d occupied; %d iterations" % (est["active_bricks"], est["occupied_bricks"], est["iterations"]))
    assert lines[-1] == "%d vertices, %d faces -> %sbigmesh.ply" % (len(v), len(f), root)
    assert main(base + ["--mesh-band", "2", "--mesh-trim", "9", "--mesh-out", root + "m2.ply"]) == 0
    capsys.readouterr()
    e2 = ctx.poisson_mesh_banded(sx, sn, 7, trim_cells=9, band_bricks=2)
    assert same_bits(pr.read_ply_mesh(root + "m2.ply")[0], e2[0])
    assert main(base + ["--mesh-band", "--mesh-trim", "8"]) == 1
    assert "trim_cells" in capsys.readouterr().out
    assert main([root + "config.yml", "--mls-radius", "10", "--mesh-depth", "11", "--mesh-band"]) == 1
    assert "depth" in capsys.readouterr().out
    assert main(base + ["--mesh-band", "--mesh-samples-per-node"]) == 1
    assert "samples_per_node" in capsys.readouterr().out
