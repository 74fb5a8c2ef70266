"""The numpy restatement of the density-adaptive Poisson splat (tests/poisson_density_restatement.py) held to hand-worked
answers, without a GPU: one sample whose every figure is written out, the mass of the combined field, the prolongation on a constant,
the single-level limit against f7's own restatement, and the two thinned spheres end to end.  tests/test_gpu_poisson_density.py holds the
kernels to this restatement."""
import numpy as np
import pytest

import poisson_density_restatement as pd
import poisson_restatement as pr

CLOSED = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0, edge_without_opposite=0, edges_not_in_two_faces=0, unused_vertices=0, euler=2)


def test_one_sample_at_a_kernel_node_centre():
    """Two samples at (0, 0, 0) and (8, 8, 8), scale 8, depth 5: side 64, o = -28, h = 2; kernel depth 3: hk = 8, so the samples sit at
    3.5 and 4.5 kernel steps from o: the centres of the kernel nodes (3, 3, 3) and (4, 4, 4).  Each counts itself alone: rho = 1, w = 1 / 64.
    samples_per_node = 1 / 8: value = 3 + 1/2 log2(8) = 4.5, so lo = 4, fr = 1/2 and alpha = 1 / 128 at levels 4 and 5.
    Level 4 (h_4 = 4): sample 0 at 7 steps, half way between nodes 6 and 7 on every axis: eight nodes (6..7)^3, weight 1 / 8 each,
    llrint(1/8 . 1/128 . 2^32) = 2^22 on the z component (n^ = +z).  Level 5 (h = 2): 14 steps, nodes (13..14)^3, the same 2^22.
    Sample 1 (n^ = -z): nodes (8..9)^3 at level 4, (17..18)^3 at level 5, -2^22.  Level 3 stays empty."""
    xyz = np.array([[0, 0, 0], [8, 8, 8]], np.float32)
    nrm = np.array([[0, 0, 1, 0], [0, 0, -1, 0]], np.float32)
    R = pd.rhs_of(xyz, nrm, 5, 8.0, 0, 0.125)
    assert np.array_equal(R["o"], [-28.0, -28.0, -28.0]) and R["h"] == 2.0 and R["kd"] == 3
    assert np.array_equal(R["rho"], [1.0, 1.0]) and np.array_equal(R["w"], [1.0 / 64.0] * 2)
    assert np.array_equal(R["value"], [4.5, 4.5]) and np.array_equal(R["d"], [4.5, 4.5])
    assert not R["V"][3].any()
    for L, first in ((4, (6, 8)), (5, (13, 17))):
        want = np.zeros_like(R["V"][L])
        for s, sign in ((0, 1), (1, -1)):
            a = first[s]
            want[2, a:a + 2, a:a + 2, a:a + 2] = sign * 2 ** 22
        assert np.array_equal(R["V"][L], want) and R["V"][L].dtype == np.int64
        assert np.array_equal(R["cnt"][L], (want[2] != 0).astype(np.int64))
    # the combined field at one finest node of sample 0's own eight: its own 2^22 2^-32 = 2^-10, and the level-4 node (6, 6, 6) prolonged
    # (2^-10 / 8 = 2^-13 on the nodes (6..7)^3, 0 around them): fine node 13 is the odd child of coarse 6 (near 6, far 7), both hold
    # 2^-13, so every axis gives 2^-13 and U = 2^-10 + 2^-13
    assert R["U"][2, 13, 13, 13] == 2.0 ** -10 + 2.0 ** -13
    # fine node 12 is the even child of coarse 6 (near 6, far 5 = 0): 0.75 per axis; no splat of its own at level 5
    assert R["U"][2, 12, 12, 12] == 0.75 ** 3 * 2.0 ** -13 and not R["U"][:2].any()
    assert R["occ"].sum() == 2 and R["occ"][14, 14, 14] == 1 and R["occ"][18, 18, 18] == 1
    # at samples_per_node = 2 the value is 3 - 1/2 and the clamp holds the sample on level 3 alone
    R2 = pd.rhs_of(xyz, nrm, 5, 8.0, 0, 2.0)
    assert np.array_equal(R2["value"], [2.5, 2.5]) and np.array_equal(R2["d"], [3.0, 3.0]) and not R2["V"][4].any() and not R2["V"][5].any()
    assert R2["V"][3][2, 3, 3, 3] == 2 ** 26 and np.count_nonzero(R2["V"][3]) == 2       # weight 1 on the one node: 1/64 2^32


def test_prolongation_of_a_constant():
    """away from the border the two weights add up to 1; at a border plane the far node lies outside: 0.75 per clipped axis"""
    P = pd.prolong(np.full((4, 4, 4), 3.0))
    assert P.shape == (8, 8, 8) and (P[1:-1, 1:-1, 1:-1] == 3.0).all()
    assert (P[0, 1:-1, 1:-1] == 2.25).all() and (P[1:-1, -1, 1:-1] == 2.25).all() and (P[1:-1, 1:-1, 0] == 2.25).all()
    assert (P[0, 0, 1:-1] == 0.75 * 2.25).all() and P[-1, -1, -1] == 0.75 * (0.75 * 2.25)
    # one node: 0.75 on its two children, 0.25 on the next node either side, along x only (axis 2)
    A = np.zeros((4, 4, 4))
    A[1, 2, 1] = 1.0
    Q = pd.prolong(A)
    assert np.array_equal(Q[2, 4, :6], np.array([0.0, 0.25, 0.75, 0.75, 0.25, 0.0]) * (0.75 * 0.75))
    assert Q.sum() == 8.0


def test_mass_of_the_combined_field():
    """P multiplies a grid's sum by 8 where nothing is clipped, the normalisation divides by 8 per level: sum over the nodes of U_depth[a] =
    sum w_s n^_a.  scale 2 keeps every level's support (levels >= 3) a node away from the border.  Each of the at most 16 contributions of a
    sample is off by half a unit 2^-33 at most; the fp64 sums round far below that."""
    rng = np.random.default_rng(8)
    d = rng.normal(size=(4000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = 20.0 * rng.uniform(size=4000) ** 2.0                                        # dense in the middle, thin outside: every level is used
    xyz, nrm = pr._with_normals(np.array([5.0, -3.0, 40.0]) + d * r[:, None], d)
    R = pd.rhs_of(xyz, nrm, 6, 2.0, 0, 2.0)
    used = [L for L in range(3, 7) if R["V"][L].any()]
    want = (R["w"][:, None] * R["nh"]).sum(0)
    got = R["U"].reshape(3, -1).sum(1)
    print("levels in use %s, d %.3f .. %.3f; sum U %s, sum w n^ %s" % (used, R["d"].min(), R["d"].max(), got, want))
    assert len(used) >= 3 and R["d"].min() < 4.0
    assert np.abs(got - want).max() <= 16 * len(xyz) * 2.0 ** -33 + 1e-13
    # without the power of 8 a coarse splat weighs 8 times too much per level
    raw = sum(R["V"][L].reshape(3, -1).sum(1).astype(np.float64) / pd.FIX * 8.0 ** (6 - L) for L in range(3, 7))
    assert np.abs(raw - want).max() > 1e-3


def test_single_level_is_f7s_splat_of_weighted_normals():
    """samples_per_node small enough that every d_s = depth: one level, alpha = w_s, and b is f7's right-hand side of the normals scaled by
    w_s within f7's fixed-point bound"""
    xyz, nrm = pr.sphere_samples(5000)
    R = pd.rhs_of(xyz, nrm, 5, 1.1, 0, 1e-6)
    assert (R["d"] == 5.0).all() and not R["V"][3].any() and not R["V"][4].any()
    V, occ, cnt = pr.splat(R["p"], R["nh"] * R["w"][:, None], R["o"], R["h"], 5)
    b_ref = pr.rhs(V)
    err, bound = np.abs(R["b"] - b_ref), pr.rhs_fixed_point_bound(cnt, b_ref)
    print("single level: max |b - f7's| %.3e, largest err / bound %.3f, max |b| %.3e" % (err.max(), (err / bound).max(), np.abs(b_ref).max()))
    assert (err <= bound).all() and err.max() > 0.0 and np.abs(b_ref).max() > 1e3 * err.max()
    assert np.array_equal(occ, R["occ"]) and np.array_equal(cnt, R["cnt"][5])


@pytest.mark.parametrize("name", ["A", "B"])
def test_thinned_sphere_end_to_end(name):
    """Setups A (depth 6, the upper hemisphere thinned to 3 %) and B (depth 5, 10 %): the surfaces are closed and oriented with Euler
    characteristic 2, and the sparse side's largest radial error stays below 1 h: the cap that separates the repaired surface (0.654 h /
    0.266 h here) from the caved-in one of the plain splat (21.3 h / 8.78 h)."""
    xyz, nrm = pd.setup_samples(name)
    depth = pd.SETUPS[name]["depth"]
    assert (len(xyz), int((nrm[:, 2] >= 0).sum())) == {"A": (30792, 856), "B": (32905, 2969)}[name]
    R = pd.reconstruct(xyz, nrm, depth, 1.1, 0, 2.0)
    Q = pr.reconstruct(xyz, nrm, depth, 1.1)
    (s, s_rms), (dn, dn_rms) = pd.side_errors(R["verts"], R["h"])
    (ps, ps_rms), (pdn, _) = pd.side_errors(Q["verts"], Q["h"])
    print("setup %s (depth %d): sparse side max %.3f h (rms %.3f), plain f7 %.2f h (rms %.2f); dense side %.3f h, plain %.3f h; %.1f %% of the samples "
          "below the finest level, least depth %.2f" % (name, depth, s, s_rms, ps, ps_rms, dn, pdn, 100.0 * (R["d"] < depth).mean(), R["d"].min()))
    assert pr.manifold_report(R["verts"], R["faces"]) == CLOSED and pr.manifold_report(Q["verts"], Q["faces"]) == CLOSED
    assert s < 1.0 and dn < 1.0
    assert ps > 1.0
