"""The banded GPU Poisson call with the density-adaptive splat (csrc/k_poisson_band_density.hip) against its numpy restatement
(tests/poisson_band_density_restatement.py, held to f14's and f16's restatements without a GPU in tests/test_poisson_band_density_cpu.py):
with the restatement's depths handed in the bricks are its integers and occ, rho, w, g and b_f its bytes; the depths themselves within f14's
cap on log2; the coarse problem is the library's own density-adaptive one at depth - 1; the weighted iso-value; the whole call on the thinned
sphere against the restatement and against the plain banded call; the refusals; the API / CLI switch.  Grids of 64^3 and one of 128^3.

Figures (MI355X; 28 tests in 12.4 s, the slowest 2.5 s):
  stage            bricks, occ, rho, w, d, g and all S 512 doubles of b_f equal on every input: A (D = 6, 502 of 512 bricks, P(W) non-zero at 4 263 nodes
                   off the band), sparse (D = 7, 432 of 4096, 609 400 such nodes), plate (192 of 512, no sample at level D), corners (54 of 512)
  depths           max |d - restatement| within 1e-12 over kernel_depth {3, 4, 0} x samples_per_node {0.5, 2, 3, 50}; b_f then differs by nothing
  iso              |GPU - restatement on the GPU's chi| 0 (bound 1.7e-12); the unweighted mean of the same chi -6.91e-4 against -6.46e-4
  whole call       A, depth 6, trim 4: 46 284 vertices, 92 564 faces (the restatement's counts), 43 iterations 8.569e-1 -> 3.840e-5, coarse 10 cycles;
                   sparse side max 0.6538 h (rms 0.3255), dense side 0.3428 h, the restatement's in every printed digit; the plain banded call
                   6.9412 h / 0.3507 h; 1 322 of 30 792 samples below depth 6, least 3.224
  rig              run() -> mesh(depth=7, band_bricks=1, band_samples_per_node=2): 43 977 faces, 444 bricks, 39 iterations, 1 281 of 55 303 samples
                   below depth 7, least 4.300"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import poisson_band_density_restatement as pbd
import poisson_band_restatement as pb
import poisson_density_restatement as pd
import poisson_restatement as pr
from reconstruction_amd import RsmError, _lib, synth

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
    """two samples, each in a corner cell of the grid they span (f16's fixture)"""
    return pr._with_normals(np.array([[-3.0, 2.0, 10.0], [5.0, 10.0, 18.0]]), np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]]))


def random_cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform([-40.0, 10.0, 300.0], [24.0, 74.0, 364.0], size=(n, 3))
    d = rng.normal(size=(n, 3))
    return pr._with_normals(xyz, d / np.linalg.norm(d, axis=1)[:, None])


BAD_X = np.array([[np.nan, 0, 0], [1, 2, 3], [np.inf, 0, 0], [5, 5, 5], [0, -np.inf, 1]], np.float32)
BAD_N = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0], [np.nan, 0, 0, 0], [1, 0, 0, 0]], np.float32)


def with_bad_rows(xyz, nrm):
    """rows that take no part at the front (2), in the middle (2) and at the end (1); the mask of the original rows"""
    m = len(xyz) // 2
    x = np.concatenate([BAD_X[:2], xyz[:m], BAD_X[2:4], xyz[m:], BAD_X[4:]])
    n = np.concatenate([BAD_N[:2], nrm[:m], BAD_N[2:4], nrm[m:], BAD_N[4:]])
    keep = np.ones(len(x), bool)
    keep[[0, 1, 2 + m, 3 + m, len(x) - 1]] = False
    return x, n, keep


# name -> (samples, depth, scale, band_bricks, samples_per_node)
INPUTS = {"A": (lambda: pd.setup_samples("A"), 6, 1.1, 1, 2.0), "sparse": (lambda: pb.sparse_fixture()[0], 7, 3.0, 1, 2.0),
          "plate": (lambda: pr.plate_samples(20000), 6, 1.0, 1, 50.0), "corners": (corner_samples, 6, 1.0, 2, 2.0),
          "all_active": (lambda: pd.setup_samples("A"), 6, 1.1, 2, 2.0)}


def samples_of(name):
    return cached(("samples", name), INPUTS[name][0])


def coarse_field(depth):
    """any coarse field: the guess is its prolongation"""
    return cached(("chi_c", depth), lambda: np.random.default_rng(31).normal(size=((1 << depth) >> 1,) * 3).astype(np.float32))


def mixed_depths(n, depth):
    """The sparse fixture is evenly and densely sampled: its own depths are all D, nothing reaches the coarser levels and P(W) is zero.  These
    rows spread it over the levels 3..D, so that level-D sums, every coarser level and P(W) beyond the band's faces all take part."""
    d = np.full(n, float(depth))
    d[::5] = depth - 0.5
    d[::7] = 4.5
    d[::11] = 3.0
    d[::13] = depth - 1.0
    return d


def ref_of(name, kd=0, spn=None):
    xyz, nrm = samples_of(name)
    depth, scale, band = INPUTS[name][1:4]
    spn = INPUTS[name][4] if spn is None else spn
    d = mixed_depths(len(xyz), depth) if name == "sparse" else None
    return cached(("ref", name, kd, spn), lambda: pbd.band_density_rhs(xyz, nrm, depth, scale, band, kd, spn, d=d))


def check_stage(ctx, xyz, nrm, depth, scale, band, spn, kd, R, label):
    """with the restatement's d handed in: the bricks are its integers; occ, rho, w, d, g and b_f its bytes"""
    ok = R["ok"]
    d_rows = pd.expand(R["d"], ok)
    chi_c = coarse_field(depth)
    G = ctx.poisson_band_rhs_weighted(xyz, nrm, depth, scale, band, spn, kd, depth_in=d_rows, chi_c=chi_c)
    bricks = R["bricks"]
    off = ~R["mask"]
    print("%s: depth %d, %d of %d bricks active, %d occupied; n %d (%d valid), kd %d, spn %g: %d samples below depth, least d %.4f; max |b_f| %.3e; "
          "level-D sums non-zero at %d nodes, P(W) non-zero at %d nodes off the band"
          % (label, depth, len(bricks), R["active"].size, int(R["occupied"].sum()), len(xyz), ok.sum(), R["kd"], spn, (R["d"] < depth).sum(), R["d"].min(),
             np.abs(G["b"]).max(), int(np.count_nonzero(R["V_D"].any(0))), int(np.count_nonzero(R["U"][:, off].any(0)))))
    assert G["bricks"].dtype == np.int32 and np.array_equal(G["bricks"], bricks)
    assert G["counts"] == (int(ok.sum()), int((~ok).sum()), len(bricks), int(R["occupied"].sum()))
    assert np.array_equal(G["grid"], np.array([R["o"][0], R["o"][1], R["o"][2], R["h"]]))
    assert same_bits(G["occ"], pb.to_bricks(R["occ"], bricks))
    assert same_bits(G["rho"], pd.expand(R["rho"], ok)) and same_bits(G["w"], pd.expand(R["w"], ok)) and same_bits(G["d"], d_rows)
    assert same_bits(G["g"], pb.to_bricks(pb.guess(chi_c), bricks))
    assert np.abs(G["b"]).max() > 0 and same_bits(G["b"], pb.to_bricks(R["b"], bricks))
    return G


# ---- 1: the stage, to the bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "sparse", "plate", "corners"])
def test_rhs_stage_is_the_restatements_bits(ctx, name):
    """A: most of the grid is band.  sparse (with mixed_depths): 432 of 4096 bricks, so most band faces have inactive neighbours and b_f reads
    P(W) off the band.
    plate at scale 1 with 50 samples per node: bricks on the grid's faces, P reads outside the coarse grid, the coarse splats are clipped, no
    sample reaches level D.  corners: two samples in the grid's corner cells."""
    xyz, nrm = samples_of(name)
    depth, scale, band, spn = INPUTS[name][1:]
    R = ref_of(name)
    check_stage(ctx, xyz, nrm, depth, scale, band, spn, 0, R, name)
    B = R["active"].shape[0]
    if name == "sparse":
        assert len(R["bricks"]) == 432 and B ** 3 == 4096 and R["U"][:, ~R["mask"]].any() and R["V_D"].any() and set(np.unique(R["d"])) == {3.0, 4.5, 6.0, 6.5, 7.0}
    if name == "plate":
        bx = R["bricks"] % B
        assert (bx == 0).any() and (bx == B - 1).any() and not R["V_D"].any() and R["d"].max() < depth - 1
    if name == "corners":
        assert {0, B ** 3 - 1} <= set(R["bricks"].tolist()) and int(R["occupied"].sum()) == 2
    if name == "A":
        assert 0 < len(R["bricks"]) < B ** 3 and R["V_D"].any() and 0 < (R["d"] < depth).sum() < len(R["d"])


def test_rows_that_take_no_part(ctx):
    """NaN, inf and zero-normal rows at the front, in the middle and at the end: every figure of the valid samples stays"""
    xyz, nrm = samples_of("A")
    x, n, keep = with_bad_rows(xyz, nrm)
    R = dict(ref_of("A"), ok=keep)
    G = check_stage(ctx, x, n, 6, 1.1, 1, 2.0, 0, R, "A with rows that take no part")
    assert G["counts"][1] == 5 and len(x) % 256 != 0


@pytest.mark.parametrize("n", [255, 256, 257])
def test_rhs_stage_with_constructed_depths(ctx, n):
    """depth_in holds 3.0, D - 1 and D exactly, values strictly between D - 1 and D, below 3 and above D (clamped) and integers in between; the
    last block of samples is full, one short, one over"""
    D = 6
    xyz, nrm = random_cloud(n, 60 + n)
    din = np.resize(np.array([3.0, 5.0, 6.0, 5.5, 2.5, 100.0, 4.0, 5.25, -1.0, 6.0 - 2.0 ** -40, 5.0 + 2.0 ** -45, 3.75, 5.0 - 2.0 ** -40]), n)
    x, nr, keep = with_bad_rows(xyz, nrm)
    rows = np.zeros(len(x))
    rows[keep] = din
    R = pbd.band_density_rhs(x, nr, D, 1.1, 1, 0, 2.0, d=rows)
    assert set(np.unique(R["d"])) >= {3.0, 4.0, 5.0, 5.5, 6.0} and R["d"].min() == 3.0 and R["d"].max() == 6.0 and R["V_D"].any() and R["W"].any()
    G = ctx.poisson_band_rhs_weighted(x, nr, D, 1.1, 1, 2.0, 0, depth_in=rows, chi_c=coarse_field(D))
    ok = R["ok"]
    print("n %d: %d valid, %d bricks, level-D sums at %d nodes, max |b_f| %.3e" % (n, ok.sum(), len(R["bricks"]), int(np.count_nonzero(R["V_D"].any(0))), np.abs(G["b"]).max()))
    assert ok.sum() == n and np.array_equal(G["bricks"], R["bricks"]) and G["counts"][:2] == (n, 5)
    assert same_bits(G["d"], pd.expand(R["d"], ok)) and same_bits(G["rho"], pd.expand(R["rho"], ok)) and same_bits(G["w"], pd.expand(R["w"], ok))
    assert same_bits(G["occ"], pb.to_bricks(R["occ"], R["bricks"])) and same_bits(G["b"], pb.to_bricks(R["b"], R["bricks"]))


def test_every_brick_active_is_the_gpus_own_dense_right_hand_side(ctx):
    """D = 6 with every brick active: b_f, scattered back to the dense layout, is byte for byte what the density-adaptive dense call computes"""
    xyz, nrm = samples_of("all_active")
    R = ref_of("all_active")
    assert len(R["bricks"]) == 512
    d_rows = pd.expand(R["d"], R["ok"])
    G = check_stage(ctx, xyz, nrm, 6, 1.1, 2, 2.0, 0, R, "all active")
    grid, b, occ, counts, rho, w, d = ctx.poisson_rhs_weighted(xyz, nrm, 6, 1.1, 2.0, 4, depth_in=d_rows)
    assert same_bits(pb.from_bricks(G["b"], G["bricks"], 6), b) and same_bits(pb.from_bricks(G["occ"], G["bricks"], 6), occ)
    assert same_bits(G["rho"], rho) and same_bits(G["w"], w) and same_bits(G["d"], d) and np.array_equal(G["grid"], grid)


def test_coarse_problem_is_the_density_adaptive_one_at_the_coarser_depth(ctx):
    """without a caller's coarse field the guess is the prolongation of the library's own solve of f14's problem at depth - 1 with kernel depth
    K and d = min(d, D - 1); and one sample gives nothing to mesh"""
    xyz, nrm = samples_of("A")
    R = ref_of("A")
    d_rows = pd.expand(R["d"], R["ok"])
    G = ctx.poisson_band_rhs_weighted(xyz, nrm, 6, samples_per_node=2.0, depth_in=d_rows)
    bc = ctx.poisson_rhs_weighted(xyz, nrm, 5, 1.1, 2.0, 4, depth_in=np.minimum(d_rows, 5.0))[1]
    assert same_bits(bc, R["b_c"])
    chi_c = ctx.poisson_solve(bc)[0]
    assert G["status"] == 0 and same_bits(G["g"], pb.to_bricks(pb.guess(chi_c), R["bricks"])) and same_bits(G["b"], pb.to_bricks(R["b"], R["bricks"]))
    one = pr._with_normals(np.array([[1.0, 2.0, 3.0]]), np.array([[0.0, 0.0, 1.0]]))       # a single sample: side = 0
    for x, n, valid in (one + (1,), (np.zeros((0, 3), np.float32), np.zeros((0, 4), np.float32), 0), (np.tile(BAD_X, (3, 1)), np.tile(BAD_N, (3, 1)), 0)):
        E = ctx.poisson_band_rhs_weighted(x, n, 6)
        assert E["grid"][3] == 0.0 and E["counts"] == (valid, len(x) - valid, 0, 0) and len(E["bricks"]) == 0 and not E["rho"].any() and not E["w"].any() and not E["d"].any()
        v, f, st = ctx.poisson_mesh_banded_weighted(x, n, 6)
        assert v.shape == (0, 3) and f.shape == (0, 3) and st["status"] == 0 and st["n_valid"] == valid and st["active_bricks"] == 0
        assert st["h"] == 0.0 and st["sum_w"] == 0.0 and st["n_below_depth"] == 0


# ---- 2: the depths without depth_in ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kd", [3, 4, 0])
@pytest.mark.parametrize("spn", [0.5, 2.0, 3.0, 50.0])
def test_depths_of_the_library(ctx, kd, spn):
    """the GPU's own d within 1e-12 of the restatement's (f14's cap for the two log2 implementations); with those depths handed back to the
    restatement b_f differs by nothing; the stats of the whole call are those of these samples"""
    xyz, nrm = samples_of("A")
    R = ref_of("A", kd, spn)
    ok = R["ok"]
    chi_c = coarse_field(6)
    G = ctx.poisson_band_rhs_weighted(xyz, nrm, 6, 1.1, 1, spn, kd, chi_c=chi_c)
    gap = np.abs(G["d"][ok] - R["d"]).max()
    R2 = pbd.band_density_rhs(xyz, nrm, 6, 1.1, 1, kd, spn, d=G["d"])
    print("A kd %d spn %g: max |d - restatement| %.3e; %d samples below depth 6, %d below 5, least %.4f" % (kd, spn, gap, (R["d"] < 6).sum(), (R["d"] < 5).sum(), R["d"].min()))
    assert same_bits(G["rho"], pd.expand(R["rho"], ok)) and same_bits(G["w"], pd.expand(R["w"], ok))
    assert gap <= 1e-12 and not G["d"][~ok].any()
    assert same_bits(G["b"], pb.to_bricks(R2["b"], R2["bricks"])) and np.array_equal(G["bricks"], R2["bricks"])
    if spn == 50.0:
        assert R["d"].max() < 5.0 and not R["V_D"].any()                                      # b_f is all prolongation
    st = ctx.poisson_mesh_banded_weighted(xyz, nrm, 6, trim_cells=0, samples_per_node=spn, kernel_depth=kd, max_iterations=1)[2]
    assert st["kernel_depth"] == R["kd"] == (kd or 4) and st["min_sample_depth"] == G["d"][ok].min() and st["n_below_depth"] == int((G["d"][ok] < 6).sum())
    assert abs(st["sum_w"] - R["w"].sum()) <= len(R["w"]) * 2.0 ** -52 * R["w"].max()


# ---- 3: the iso-value --------------------------------------------------------------------------------------------------------------------------
def test_iso_value_is_the_weighted_mean_of_chi_at_the_valid_samples(ctx):
    """The stages chained by hand give the whole call's field, so its iso-value is held to the restatement's rule on that field.  Both sides sum
    n fp64 terms w chi bounded by max w max|chi| in their own order and divide by sum w >= n min w: the means agree within n 2^-52 max|chi|
    (max w / min w), f14's bound."""
    xyz, nrm = samples_of("A")
    R = ref_of("A")
    G = ctx.poisson_band_rhs_weighted(xyz, nrm, 6, samples_per_node=2.0)
    bricks = G["bricks"]
    chi_c = ctx.poisson_solve(ctx.poisson_rhs_weighted(xyz, nrm, 5, 1.1, 2.0, 4, depth_in=np.minimum(G["d"], 5.0))[1])[0]
    assert same_bits(G["g"], pb.to_bricks(pb.guess(chi_c), bricks))
    chi = ctx.poisson_band_solve(bricks, 6, G["b"], G["g"], chi_c)[0]
    v, f, st = ctx.poisson_mesh_banded_weighted(xyz, nrm, 6, trim_cells=0, samples_per_node=2.0)
    dense = pb.from_bricks(chi, bricks, 6)
    n = len(R["p"])
    assert same_bits(G["w"][R["ok"]], R["w"])
    iso = pbd.iso_value(dense, R["p"], R["w"], R["o"], R["h"])
    plain = pr.iso_value(dense, R["p"], R["o"], R["h"])
    bound = n * 2.0 ** -52 * np.abs(chi).max() * (R["w"].max() / R["w"].min())
    print("A: iso %.17g, restatement on the GPU's chi %.17g, difference %.3e, bound %.3e; the unweighted mean %.17g" % (st["iso"], iso, abs(st["iso"] - iso), bound, plain))
    assert st["n_valid"] == n and abs(st["iso"] - iso) <= bound and abs(plain - iso) > 100.0 * bound
    sv, sf = ctx.band_iso_mesh(bricks, 6, chi, st["iso"], G["grid"])
    assert len(f) > 1000 and same_bits(sv, v) and same_bits(sf, f)


# ---- 4: the whole call ---------------------------------------------------------------------------------------------------------------------------
def whole_call(ctx):
    def make():
        xyz, nrm = samples_of("A")
        return xyz, nrm, ctx.poisson_mesh_banded_weighted(xyz, nrm, 6, trim_cells=4, samples_per_node=2.0)
    return cached("whole_call", make)


def test_whole_call_on_the_thinned_sphere(ctx):
    """Closed, oriented, manifold; the side errors within 0.005 h of the restatement's (f16's bound between its GPU and restatement whole
    calls); the sparse side strictly better than the plain banded call's on the same cloud: the contrast the call exists for."""
    xyz, nrm, (v, f, st) = whole_call(ctx)
    R = cached("whole_ref", lambda: pbd.reconstruct(xyz, nrm, 6, band_bricks=1, trim_cells=4, samples_per_node=2.0))
    (gs, gs_rms), (gd, gd_rms) = pd.side_errors(v, st["h"])
    (rs, rs_rms), (rd, rd_rms) = pd.side_errors(R["verts"], R["h"])
    pv, pf, pst = ctx.poisson_mesh_banded(xyz, nrm, 6, trim_cells=4)
    (ps, _), (pd_, _) = pd.side_errors(pv, pst["h"])
    print("setup A depth 6: %d vertices, %d faces (restatement %d, %d); %d of 512 bricks; coarse %d cycles to %.2e; band %d iterations %.3e -> %.3e "
          "(restatement %d); sparse side max %.4f h (rms %.4f), restatement %.4f (%.4f); dense side %.4f (%.4f), restatement %.4f (%.4f); the plain "
          "banded call %.4f / %.4f; %d of %d samples below depth 6, least %.3f"
          % (len(v), len(f), len(R["verts"]), len(R["faces"]), st["active_bricks"], st["coarse_cycles"], st["coarse_residual"], st["iterations"],
             st["residual_before"], st["residual"], R["iterations"], gs, gs_rms, rs, rs_rms, gd, gd_rms, rd, rd_rms, ps, pd_, st["n_below_depth"], st["n_valid"],
             st["min_sample_depth"]))
    assert st["status"] == 0 and st["converged"] and st["N"] == 64 and st["h"] == R["h"] and st["origin"] == tuple(R["o"])
    assert st["active_bricks"] == len(R["bricks"]) and st["occupied_bricks"] == int(R["occupied"].sum()) and st["kernel_depth"] == 4
    assert pr.manifold_report(v, f) == CLOSED and pr.face_orientation_min(v, f) > 0.0
    assert abs(gs - rs) <= 0.005 and abs(gd - rd) <= 0.005
    assert gs < ps


def test_two_calls_and_both_entries_return_the_same_bytes(ctx):
    xyz, nrm, (v1, f1, s1) = whole_call(ctx)
    v2, f2, s2 = ctx.poisson_mesh_banded_weighted(xyz, nrm, 6, trim_cells=4, samples_per_node=2.0)
    assert same_bits(v1, v2) and same_bits(f1, f2) and s1 == s2 and len(f1) > 1000
    dx, dn = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
    nv, nf, s3 = ctx.poisson_mesh_banded_weighted_device(dx.data_ptr(), dn.data_ptr(), len(xyz), 6, trim_cells=4, samples_per_node=2.0)
    assert (nv, nf) == (len(v1), len(f1)) and s3 == s1
    dv = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    df = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    ctx.poisson_last_mesh_device(dv.data_ptr(), df.data_ptr())
    torch.cuda.synchronize()
    assert dv.cpu().numpy().tobytes() == v1.tobytes() and df.cpu().numpy().tobytes() == f1.tobytes()
    r1, r2 = ctx.poisson_band_rhs_weighted(xyz, nrm, 6, samples_per_node=2.0), ctx.poisson_band_rhs_weighted(xyz, nrm, 6, samples_per_node=2.0)
    assert all(same_bits(np.asarray(r1[k]), np.asarray(r2[k])) for k in ("grid", "bricks", "b", "occ", "g", "rho", "w", "d"))


# ---- 5: refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_invalid_parameters_are_named(ctx):
    xyz, nrm = random_cloud(300, 3)
    dx, dn = torch.from_numpy(xyz).cuda(), torch.from_numpy(nrm).cuda()
    cases = ((dict(kernel_depth=6), "kernel_depth"), (dict(kernel_depth=2), "kernel_depth"), (dict(depth=7, kernel_depth=7), "kernel_depth"),
             (dict(samples_per_node=0.0), "samples_per_node"), (dict(samples_per_node=float("nan")), "samples_per_node"),
             (dict(depth=5), "depth"), (dict(depth=11), "depth"), (dict(trim_cells=8), "trim_cells"), (dict(trim_cells=16, band_bricks=2), "trim_cells"),
             (dict(band_bricks=0), "band_bricks"), (dict(band_bricks=5), "band_bricks"), (dict(max_iterations=0), "max_iterations"),
             (dict(scale=0.5), "scale"), (dict(rel_residual=0.0), "rel_residual"), (dict(max_cycles=0), "max_cycles"))
    for kw, word in cases:
        with pytest.raises(RsmError, match=word):
            ctx.poisson_mesh_banded_weighted(xyz, nrm, **{**dict(depth=6), **kw})
        with pytest.raises(RsmError, match=word):
            ctx.poisson_mesh_banded_weighted_device(dx.data_ptr(), dn.data_ptr(), len(xyz), **{**dict(depth=6), **kw})
    assert ctx.poisson_mesh_banded_weighted(xyz, nrm, 6, kernel_depth=5, trim_cells=7)[2]["kernel_depth"] == 5     # D - 1 and 8 band_bricks - 1 are allowed
    for kw, word in ((dict(kernel_depth=6), "kernel_depth"), (dict(samples_per_node=0.0), "samples_per_node"), (dict(band_bricks=0), "band_bricks")):
        with pytest.raises(RsmError, match=word):
            ctx.poisson_band_rhs_weighted(xyz, nrm, 6, **kw)
    for bad in (np.nan, np.inf):
        din = np.full(300, 4.0)
        din[299] = bad
        with pytest.raises(RsmError, match=r"depth_in\[299\]"):
            ctx.poisson_band_rhs_weighted(xyz, nrm, 6, depth_in=din)
    prm, bpr, dpr = _lib.PoissonParams(6, 1.1, 0.5, 1, 0), _lib.PoissonBandParams(1, 1), _lib.PoissonDensityParams(0, 2.0)
    nv, nf = C.c_int64(), C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = ctx._lib
    for fn, x, n in ((lib.rsm_poisson_mesh_banded_weighted, p(xyz), p(nrm)), (lib.rsm_poisson_mesh_banded_weighted_device, dx.data_ptr(), dn.data_ptr())):
        for params, word in (((None, C.byref(bpr), C.byref(dpr)), "params is NULL"), ((C.byref(prm), None, C.byref(dpr)), "band params is NULL"),
                             ((C.byref(prm), C.byref(bpr), None), "density params is NULL")):
            assert fn(ctx._h, x, n, 300, *params, C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
            assert word in ctx._lib.rsm_last_error(ctx._h).decode()
        assert fn(ctx._h, None, n, 300, C.byref(prm), C.byref(bpr), C.byref(dpr), C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
        assert fn(ctx._h, x, n, 300, C.byref(prm), C.byref(bpr), C.byref(dpr), None, C.byref(nf), None) == _lib.RSM_E_INVALID
        assert fn(ctx._h, x, n, -1, C.byref(prm), C.byref(bpr), C.byref(dpr), C.byref(nv), C.byref(nf), None) == _lib.RSM_E_INVALID
    assert lib.rsm_stage_poisson_band_rhs_weighted(ctx._h, p(xyz), p(nrm), 300, C.byref(prm), C.byref(bpr), None, None, None, 0, 512, None, None, None, None, None, None,
                                                   None, None, None) == _lib.RSM_E_INVALID
    with pytest.raises(RsmError, match="depth"):                                             # the calls this one is built from keep their ranges
        ctx.poisson_mesh_weighted(xyz, nrm, 10)


# ---- 6: the API and the CLI ------------------------------------------------------------------------------------------------------------------------
def test_cloud_optimization_mesh_with_band_samples_per_node(ctx):
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
    v, f, st = opt.mesh(depth=7, band_bricks=1, band_samples_per_node=2)
    assert opt.mesh_result[0] is v and opt.mesh_grid_step == st["h"] and st["N"] == 128
    bv, bf, bst = ctx.poisson_mesh_banded_weighted(sx, sn, 7, trim_cells=4, band_bricks=1, samples_per_node=2.0)
    print("run() -> mesh(depth=7, band_bricks=1, band_samples_per_node=2): %d faces; %d bricks, %d iterations; %d of %d samples below depth 7, least %.3f"
          % (len(f), st["active_bricks"], st["iterations"], st["n_below_depth"], st["n_valid"], st["min_sample_depth"]))
    assert same_bits(v, bv) and same_bits(f, bf) and st == bst and len(f) > 1000 and st["kernel_depth"] == 5
    v4, f4, st4 = opt.mesh(depth=7, band_bricks=1, band_samples_per_node=3, kernel_depth=4)
    assert st4["kernel_depth"] == 4 and not same_bits(v4, v)
    with pytest.raises(ValueError, match="band_samples_per_node"):
        opt.mesh(depth=7, band_samples_per_node=2)
    with pytest.raises(ValueError, match="samples_per_node"):                                                # the refusal that stays
        opt.mesh(depth=7, band_bricks=1, samples_per_node=2)
    cv, cf, cst = opt.clean_mesh()                                                                          # the later stages run on the result
    assert cst["n_faces_in"] == len(f4) and 0 < len(cf) <= len(f4)


def test_cli_mesh_band_samples_per_node(ctx, tmp_path, capsys):
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
    assert main(base + ["--mesh-band", "--mesh-band-samples-per-node"]) == 0                               # bare: script1.mlx's 3
    out = norm(capsys.readouterr().out)
    v, f = pr.read_ply_mesh(root + "bigmesh.ply")
    blob = open(root + "bigcloud.ply", "rb").read()
    rec = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], "<f4").reshape(-1, 7)
    sx, sn = rec[:, :3].copy(), rec[:, 3:].copy()
    ev, ef, est = ctx.poisson_mesh_banded_weighted(sx, sn, 7, trim_cells=4, band_bricks=1, samples_per_node=3.0)
    assert same_bits(v, ev) and np.array_equal(f, ef) and len(f) > 1000
    lines = out.splitlines()
    assert lines[-3].startswith("Mesh time: T s (band of %d bricks around %d occupied; %d iterations" % (est["active_bricks"], est["occupied_bricks"], est["iterations"]))
    assert lines[-2].startswith("Mesh samples per node 3: density on 2^5 nodes, %d of %d samples spread below depth 7" % (est["n_below_depth"], est["n_valid"]))
    assert lines[-1] == "%d vertices, %d faces -> %sbigmesh.ply" % (len(v), len(f), root)
    assert main(base + ["--mesh-band-samples-per-node", "2", "--mesh-kernel-depth", "4", "--mesh-out", root + "m2.ply"]) == 0   # implies --mesh-band 1
    capsys.readouterr()
    e2 = ctx.poisson_mesh_banded_weighted(sx, sn, 7, trim_cells=4, band_bricks=1, samples_per_node=2.0, kernel_depth=4)
    assert same_bits(pr.read_ply_mesh(root + "m2.ply")[0], e2[0]) and not same_bits(e2[0], ev)
    assert main(base + ["--mesh-band-samples-per-node", "--mesh-kernel-depth", "7"]) == 1
    assert "kernel_depth" in capsys.readouterr().out
