"""The banded Poisson call with the density-adaptive splat without a GPU: its numpy restatement
(tests/poisson_band_density_restatement.py) held to f14's dense restatement (poisson_density_restatement) and f16's banded one
(poisson_band_restatement).  tests/test_gpu_poisson_band_density.py then holds the kernels to the restatement.

Figures (printed by the tests; DESIGN.md 9 f17 records them), setup A = pd.setup_samples("A"), 30 792 samples, 856 on the thinned side:
  all active       D = 6, band_bricks 2 (512 of 512): U_D and b_f are f14's dense restatement's bits, also with 50 samples per node, where every
                   sample lies below depth 5 and V_D is zero
  coarse problem   b_c, rho and w are pd.rhs_of's bits at depth 5 with kernel depth 4 and d = min(d, 5)
  scale            least-squares factor of the exact depth-D weighted field on the prolonged exact coarse field: 0.2530 (D = 6), 0.2508 (D = 7)
  band vs dense    D = 6, 2 samples per node, band_bricks 1 (502 of 512 bricks), float32 band solve to 4e-5 in 43 iterations:
                   max |chi_band - chi_dense| / range 1.84e-3 over the active nodes; sparse side max 0.65383 h against the dense 0.65399 h
                   (1.6e-4 h apart), dense side 0.342798 h against 0.342807 h (8.8e-6 h apart); f16's plain splat on the band: 6.94 h / 0.3507 h
                   closed, oriented, Euler characteristic 2 after trim_cells = 4 with band_bricks 1; the iso-surface stays in the band"""
import numpy as np
import pytest

import poisson_band_density_restatement as pbd
import poisson_band_restatement as pb
import poisson_density_restatement as pd
import poisson_restatement as pr

CLOSED = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0, edge_without_opposite=0, edges_not_in_two_faces=0, unused_vertices=0, euler=2)
_cache = {}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def samples():
    return cached("A", lambda: pd.setup_samples("A"))


def band_rhs(depth, band, spn=2.0):
    return cached(("rhs", depth, band, spn), lambda: pbd.band_density_rhs(*samples(), depth, 1.1, band, 0, spn))


def dense_rhs(depth, spn=2.0):
    return cached(("dense", depth, spn), lambda: pd.rhs_of(*samples(), depth, 1.1, depth - 2, spn))


def test_prolongation_at_single_nodes_is_f14s():
    """prolong_at (the cascade's expression, node by node) against f14's axis-by-axis prolongation: the same bits, faces and corners included"""
    A = np.random.default_rng(3).normal(size=(3, 8, 8, 8))
    assert same_bits(pbd.prolong_everywhere(A), pd.prolong(A))
    one = np.zeros((4, 4, 4))
    one[0, 0, 0] = 1.0
    assert pbd.prolong_at(one, np.array([0, 1, 2]), np.array([0, 0, 0]), np.array([0, 0, 0])).tolist() == [0.75 ** 3, 0.75 ** 3, 0.25 * 0.75 ** 2]


@pytest.mark.parametrize("spn", [2.0, 50.0])
def test_every_brick_active_is_f14s_dense_problem(spn):
    """the pointwise P and the order of rules 5 and 6 against f14, independently of the band; with 50 samples per node b_f is all prolongation"""
    R, F = band_rhs(6, 2, spn), dense_rhs(6, spn)
    assert len(R["bricks"]) == 512 and R["mask"].all()
    assert same_bits(R["rho"], F["rho"]) and same_bits(R["w"], F["w"]) and same_bits(R["d"], F["d"]) and R["kd"] == F["kd"] == 4
    assert same_bits(R["U"], F["U"]) and same_bits(R["b"], F["b"]) and np.array_equal(R["occ"], F["occ"]) and np.abs(R["b"]).max() > 0
    below = int((R["d"] < 6).sum())
    print("all 512 bricks active, %g samples per node: %d of %d samples below depth 6, least d %.4f, greatest %.4f" % (spn, below, len(R["d"]), R["d"].min(), R["d"].max()))
    if spn == 50.0:
        assert R["d"].max() < 5.0 and not R["V_D"].any()
    else:
        assert 0 < below < len(R["d"]) and R["V_D"].any() and R["W"].any()


def test_coarse_problem_is_f14s_at_the_coarser_depth():
    R = band_rhs(6, 1)
    xyz, nrm = samples()
    F = pd.rhs_of(xyz, nrm, 5, 1.1, 4, 2.0, d=pd.expand(np.minimum(R["d"], 5.0), R["ok"]))
    assert np.array_equal(F["o"], R["o"]) and F["h"] == 2.0 * R["h"]
    assert same_bits(F["rho"], R["rho"]) and same_bits(F["w"], R["w"]) and same_bits(F["d"], R["d_c"])
    assert same_bits(F["b"], R["b_c"]) and (R["d"] > 5.0).any() and (R["d"] < 5.0).any()


def test_mass_of_the_splat():
    """Every component of U_D summed over the whole fine grid (the band plus P(W) off it) against f14's dense restatement at depth D: two
    sums of N^3 fp64 terms, each within N^3 2^-53 sum |U| of the exact sum.  (sum w_s n^_s is printed beside it: the coarse levels' splats
    are clipped at the grid's faces, so it is larger.)"""
    R, F = band_rhs(6, 1), dense_rhs(6)
    assert 0 < len(R["bricks"]) < 512 and (~R["mask"]).any() and R["U"][:, ~R["mask"]].any()
    n3 = R["U"][0].size
    want = (R["w"][:, None] * R["nh"]).sum(0)
    for a in range(3):
        tol = 2.0 * n3 * 2.0 ** -53 * np.abs(F["U"][a]).sum()
        got, dense = R["U"][a].sum(), F["U"][a].sum()
        print("component %d: mass %.17g, dense restatement %.17g (tolerance %.3e), sum w n %.17g" % (a, got, dense, tol, want[a]))
        assert abs(got - dense) <= tol


@pytest.mark.parametrize("depth", [6, 7])
def test_fine_field_is_a_quarter_of_the_prolonged_coarse_one(depth):
    """the assertion tells 1/4 from 1/8 and 1/2: the geometric midpoints"""
    R, F = band_rhs(depth, 1), dense_rhs(depth)
    P = pb.prolong(pr.solve_exact(R["b_c"]))
    factor = float((P * pr.solve_exact(F["b"])).sum() / (P * P).sum())
    print("depth %d: least-squares factor %.4f" % (depth, factor))
    assert 0.177 < factor < 0.354


def whole():
    return cached("whole", lambda: pbd.reconstruct(*samples(), 6, band_bricks=1, trim_cells=4, samples_per_node=2.0))


def dense_whole():
    return cached("dense_whole", lambda: pd.reconstruct(*samples(), 6, samples_per_node=2.0, trim_cells=4))


# measured on the CPU (this file's header); the bounds are twice that: the margin covers the float32 band solve's stopping point
MEASURED = dict(chi=1.84e-3, sparse=1.6e-4, dense=8.8e-6)


def test_band_field_and_surface_against_the_dense_restatement():
    R, F = whole(), dense_whole()
    m = R["mask"]
    err = float(np.abs(R["chi"].astype(np.float64) - F["chi"])[m].max() / (F["chi"].max() - F["chi"].min()))
    (bs, bs_rms), (bd, bd_rms) = pd.side_errors(R["verts"], R["h"])
    (fs, _), (fd, _) = pd.side_errors(F["verts"], F["h"])
    print("depth 6: %d of 512 bricks, %d iterations from %.3e to %.3e; max |chi_band - chi_dense| / range %.3e; sparse side max %.5f h (dense %.5f), "
          "dense side %.6f h (dense %.6f); %d vertices, %d faces" % (len(R["bricks"]), R["iterations"], R["residual0"], R["residual"], err, bs, fs, bd, fd,
                                                                     len(R["verts"]), len(R["faces"])))
    assert R["status"] == 0 and 0 < len(R["bricks"]) < 512
    assert abs(fs - 0.6540) < 5e-5 and abs(fd - 0.3428) < 5e-5                              # f14's figures
    assert err <= 2.0 * MEASURED["chi"] and abs(bs - fs) <= 2.0 * MEASURED["sparse"] and abs(bd - fd) <= 2.0 * MEASURED["dense"]


def test_trimmed_surface_is_closed_and_stays_in_the_band():
    R = whole()
    assert pr.manifold_report(R["verts"], R["faces"]) == CLOSED and pr.face_orientation_min(R["verts"], R["faces"]) > 0.0
    assert pbd.surface_inside_band(R["chi"], R["iso"], R["mask"])
    plain = cached("plain", lambda: pb.reconstruct_band(*samples(), 6, band_bricks=1, trim_cells=4))
    (ps, _), _ = pd.side_errors(plain["verts"], plain["h"])
    (bs, _), _ = pd.side_errors(R["verts"], R["h"])
    print("sparse side: %.4f h with the density-adaptive splat, %.4f h with the plain one on the same band" % (bs, ps))
    assert bs < 1.0 < ps
