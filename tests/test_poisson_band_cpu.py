"""The banded finest level of the Poisson surface without a GPU: its numpy restatement (tests/poisson_band_restatement.py)
held to the dense restatement (tests/poisson_restatement.py) and to exact sine-transform solves.  tests/test_gpu_poisson_band.py then holds
the kernels to the restatement.

Figures (printed by the tests; DESIGN.md 9 f16 records them):
  scale            least-squares factor of the dense depth-D field on the prolonged depth-(D-1) field: 0.2550 (D = 6), 0.2524 (D = 7); 1/4 in
                   the continuum
  band vs dense    max |chi_band - chi_dense| / range over the active nodes, float32 band solve stopped at 4e-5: 3.1e-4 (D = 6, 504 of 512
                   bricks, 41 iterations), 1.83e-4 (D = 7, 2832 of 4096, 50 iterations)
  all active       D = 6, band_bricks 2 (512 of 512): the fp64 band solve at residual <= 1e-12 (141 iterations) against the direct solution: 2.5e-12 of the range
  sparse fixture   sphere_samples(300000), scale 3.0, D = 7: 432 of 4096 bricks active
  stall            longest run without a new best before the float32 floor: 1 (D = 6, band 1), 10 (D = 6, band 2); STALL = 20"""
import numpy as np
import pytest

import poisson_band_restatement as pb
import poisson_restatement as pr

CLOSED = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0, edge_without_opposite=0, edges_not_in_two_faces=0, unused_vertices=0, euler=2)
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def setup(depth, n, scale=1.1, band=1):
    """the sphere's band right-hand side, the exact coarse and dense fields and the guess"""
    def make():
        xyz, nrm = pr.sphere_samples(n)
        R = pb.band_rhs(xyz, nrm, depth, scale, band)
        Vc, _, _ = pr.splat(R["p"], R["nh"], R["o"], 2.0 * R["h"], depth - 1)
        R["coarse"] = pr.solve_exact(pr.rhs(Vc))
        R["dense"] = pr.solve_exact(R["b"])
        R["g"] = pb.guess(R["coarse"].astype(np.float32))
        return R
    return cached(("setup", depth, n, scale, band), make)


def test_prolongation_weights():
    """3/4 on the parent and 1/4 on its neighbour towards the fine node: a field linear in the coarse index comes back linear in the fine one
    (fine node i sits at coarse coordinate i / 2 - 1 / 4), away from the faces where the zero outside enters"""
    Nc = 8
    k, j, i = np.indices((Nc, Nc, Nc)).astype(np.float64)
    P = pb.prolong(3.0 * i - 2.0 * j + 0.5 * k + 7.0)
    fk, fj, fi = np.indices((2 * Nc,) * 3).astype(np.float64)
    want = 3.0 * (fi / 2 - 0.25) - 2.0 * (fj / 2 - 0.25) + 0.5 * (fk / 2 - 0.25) + 7.0
    assert np.abs(P - want)[1:-1, 1:-1, 1:-1].max() < 1e-12
    one = np.zeros((Nc, Nc, Nc))
    one[3, 4, 5] = 1.0                                               # [k, j, i]: its eight children get (3/4)^3, the next ring 3/4 3/4 1/4 ...
    P = pb.prolong(one)
    assert P[6, 8, 10] == 0.75 ** 3 and P[7, 9, 11] == 0.75 ** 3 and P[6, 8, 9] == 0.75 * 0.75 * 0.25 and P[5, 7, 9] == 0.25 ** 3 and P[4, 8, 10] == 0.0
    assert abs(P.sum() - 8.0) < 1e-12
    corner = np.zeros((Nc, Nc, Nc))
    corner[0, 0, 0] = 1.0                                            # at the grid's corner the neighbours outside hold 0
    assert pb.prolong(corner)[0, 0, 0] == 0.75 ** 3
    g = pb.guess(np.full((Nc, Nc, Nc), 2.0, np.float32))
    assert g.dtype == np.float32 and g[5, 6, 7] == np.float32(0.5) and g[0, 0, 0] == np.float32(0.25 * 2.0 * 0.75 ** 3)


@pytest.mark.parametrize("depth,n", [(6, 80000), (7, 300000)])
def test_dense_field_is_a_quarter_of_the_prolonged_coarse_one(depth, n):
    R = setup(depth, n)
    P = pb.prolong(R["coarse"])
    factor = float((P * R["dense"]).sum() / (P * P).sum())
    print("depth %d: least-squares factor %.4f" % (depth, factor))
    assert 0.24 <= factor <= 0.27


@pytest.mark.parametrize("depth,n,scale", [(6, 80000, 1.1), (7, 300000, 3.0)])
def test_right_hand_side_is_zero_outside_the_band(depth, n, scale):
    R = setup(depth, n) if scale == 1.1 else cached(("rhs", depth, n, scale), lambda: pb.band_rhs(*pr.sphere_samples(n), depth, scale, 1))
    assert (~R["mask"]).any() and not R["b"][~R["mask"]].any() and R["b"][R["mask"]].any()


def test_sparse_fixture_is_sparse():
    (xyz, nrm), depth, scale = pb.sparse_fixture()
    R = cached(("rhs", depth, len(xyz), scale), lambda: pb.band_rhs(xyz, nrm, depth, scale, 1))
    print("sparse fixture: %d of %d bricks active, %d occupied" % (len(R["bricks"]), R["active"].size, int(R["occupied"].sum())))
    assert 0 < len(R["bricks"]) <= 0.15 * R["active"].size
    assert np.array_equal(R["bricks"], np.sort(R["bricks"])) and R["active"].ravel()[R["bricks"]].all() and len(R["bricks"]) == int(R["active"].sum())


# the issue's figures: 3.1e-4 and 1.6e-4 of the range; twice that for another seed of rounding, not more
@pytest.mark.parametrize("depth,n,measured", [(6, 80000, 3.1e-4), (7, 300000, 1.6e-4)])
def test_band_field_against_the_dense_one(depth, n, measured):
    R = setup(depth, n)
    S = pb.band_solve(R["b"], R["g"], R["mask"], 4e-5, 200)
    m = R["mask"]
    err = float(np.abs(S["chi"].astype(np.float64) - R["dense"])[m].max() / (R["dense"].max() - R["dense"].min()))
    print("depth %d: %d of %d bricks, %d iterations from %.3e to %.3e, max |band - dense| / range %.2e" %
          (depth, len(R["bricks"]), R["active"].size, S["iterations"], S["residual0"], S["residual"], err))
    assert S["status"] == 0 and S["residual"] <= 4e-5 and S["iterations"] <= 60
    assert err <= 2.0 * measured
    assert np.array_equal(S["chi"][~m], R["g"][~m])                                         # no correction off the band


def histories():
    def make():
        out = {}
        for band in (1, 2):
            R = setup(6, 80000, band=band)
            out[band] = pb.band_pcg(R["b"], R["g"], R["mask"], 90, np.float32)
        return out
    return cached("histories", make)


def test_every_brick_active_is_the_dense_problem():
    R = setup(6, 80000, band=2)
    assert len(R["bricks"]) == 512 and R["mask"].all()
    res0, hist, chi = pb.band_pcg(R["b"], R["g"], R["mask"], 400, np.float64, stop=1e-12)
    err = float(np.abs(chi - R["dense"]).max() / (R["dense"].max() - R["dense"].min()))
    print("all 512 bricks active: fp64 band solve to %.1e in %d iterations, max |band - exact| / range %.1e" % (hist[-1], len(hist), err))
    assert hist[-1] <= 1e-12 and err <= 1e-6


def test_preconditioner_halves_the_iterations_and_the_stall_constant():
    """The symmetric Gauss-Seidel sweep against plain conjugate gradients, and STALL = twice the longest run without a new best before the
    float32 floor over the fixtures (the D = 7 ones, 1 and 6, are recorded in DESIGN.md 9 f16; the longest is D = 6 with every brick active)."""
    H = histories()
    runs = {band: pb.longest_run_without_best(H[band][1], H[band][0]) for band in H}
    R = setup(6, 80000, band=1)
    plain = pb.band_pcg(R["b"], R["g"], R["mask"], 200, np.float32, stop=4e-5, precond=False)[1]
    with_m = int(np.argmax(H[1][1] <= 4e-5)) + 1
    print("iterations to 4e-5: %d with the sweep, %d without; longest runs without a new best before the floor: %s" % (with_m, len(plain), runs))
    print("history (D = 6, band 1): " + " ".join("%.2e" % v for v in H[1][1]))
    print("history (D = 6, band 2): " + " ".join("%.2e" % v for v in H[2][1]))
    assert plain[-1] <= 4e-5 and with_m <= 0.6 * len(plain)
    assert pb.STALL == 2 * max(runs.values())
    for band in H:                                                                           # the red, black, black, red sweep: the second black pass changes nothing
        r = (R["b"] * R["mask"]).astype(np.float32)
        z3 = np.zeros_like(r)
        for colour in (0, 1, 0):
            pb._band_rbgs(z3, r, colour, R["mask"])
        assert np.array_equal(z3, pb.precondition(r, R["mask"]))


def holes_field():
    """random values on the pattern with holes, as the GPU test extracts them"""
    def make():
        bricks = pb.holes_pattern(6)
        chi = np.random.default_rng(11).normal(size=(64, 64, 64)).astype(np.float32)
        return bricks, chi, 0.1
    return cached("holes", make)


def face_set(faces, keys):
    k = np.asarray(keys)[np.asarray(faces)]
    return set(map(tuple, k.tolist()))


def test_band_extraction_equals_the_dense_one_on_whole_cells():
    """An independent reference for the brick indexing: f7's extraction of the same field on the dense grid, its faces restricted to the cells
    whose eight corners are active, as a set over the vertex keys 8 a + direction; and the vertices at equal keys are equal."""
    bricks, chi, iso = holes_field()
    mask = pb.node_mask(pb.active_of_list(bricks, 6))
    assert 0.5 < mask.mean() < 0.6                                                           # a checkerboard plus a block: holes everywhere
    v, f, keys, dkeys = pb.extract_band(chi, iso, pr.FIELD_O, pr.FIELD_H, bricks)
    dv, df, dk = pr.extract(chi, iso, pr.FIELD_O, pr.FIELD_H)
    N = 64
    a = dk // 8
    off = pr.DIRS[dk % 8]
    ijk = np.stack([a % N, (a // N) % N, a // (N * N)], 1)
    both = mask.ravel()[a] & mask[ijk[:, 2] + off[:, 2], ijk[:, 1] + off[:, 1], ijk[:, 0] + off[:, 0]]
    assert np.array_equal(np.sort(dkeys), dk[both]) and len(dkeys) > 10000                    # one vertex per crossed edge with both ends active
    assert np.array_equal(v[np.argsort(dkeys)], dv[both])
    whole = mask[:-1, :-1, :-1].copy()
    for c in range(1, 8):
        whole &= mask[(c >> 2) & 1:, (c >> 1) & 1:, c & 1:][:N - 1, :N - 1, :N - 1]
    cell_ok = np.zeros((N, N, N), bool)
    cell_ok[:-1, :-1, :-1] = whole
    # a dense face belongs to the cell of the least node among its three edges' lower ends, minus nothing: recover the cell from the face's keys
    fa = (dk[df] // 8)
    fi = np.stack([fa % N, (fa // N) % N, fa // (N * N)], 2).min(1)                          # the cell's 000 node: the componentwise least lower end
    keep = cell_ok[fi[:, 2], fi[:, 1], fi[:, 0]]
    want = face_set(df[keep], dk)
    got = face_set(f, dkeys)
    print("holes pattern: %d of %d dense faces lie in whole cells; band extraction %d faces, %d vertices" % (keep.sum(), len(df), len(f), len(v)))
    assert len(got) == len(f) == int(keep.sum()) and got == want
    counts = pb.tet_case_counts_band(chi, iso, mask)
    assert (counts[:, 1:15] > 0).all() and counts[:, 1:15].sum() > 0 and int((counts[:, 1:15] * np.array([1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1])).sum()) == len(f)


def sphere_mesh():
    return cached("sphere_mesh", lambda: pb.reconstruct_band(*pr.sphere_samples(80000), 6, 2.0, band_bricks=1, trim_cells=4))


def test_trimmed_band_mesh_equals_the_dense_extraction_and_trim():
    R = sphere_mesh()
    assert 0 < len(R["bricks"]) < 0.6 * R["active"].size
    dv, df, dk = pr.extract(R["chi"], R["iso"], R["o"], R["h"])                                # chi holds the guess off the band: the embedded field
    tv, tf = pr.trim(dv, df, R["occ"], R["o"], R["h"], 4)
    key_of = {tuple(p): i for i, p in enumerate(map(tuple, dv.tolist()))}                       # trimmed vertices back to their keys by position
    assert len(key_of) == len(dv)
    dkeys_t = dk[[key_of[tuple(p)] for p in tv.tolist()]]
    band_of = {tuple(p): i for i, p in enumerate(map(tuple, R["verts0"].tolist()))}
    bkeys_t = R["dense_keys"][[band_of[tuple(p)] for p in R["verts"].tolist()]]
    print("sphere, depth 6, scale 2: %d of %d bricks; trimmed %d vertices, %d faces (dense %d, %d)" %
          (len(R["bricks"]), R["active"].size, len(R["verts"]), len(R["faces"]), len(tv), len(tf)))
    assert len(R["faces"]) == len(tf) > 10000 and len(R["verts"]) == len(tv)
    assert face_set(R["faces"], bkeys_t) == face_set(tf, dkeys_t)


def test_trimmed_surface_is_a_closed_oriented_manifold():
    R = sphere_mesh()
    assert pr.manifold_report(R["verts"], R["faces"]) == CLOSED
    assert pr.face_orientation_min(R["verts"], R["faces"]) > 0.0
    err = pr.radial_error_h(R["verts"], R["h"])
    print("sphere, depth 6, scale 2: max radial error %.4f h" % err.max())
    assert err.max() < 0.5
    un = pr.manifold_report(R["verts0"], R["faces0"])                                       # untrimmed: the sphere never leaves its band
    assert un["edges_not_in_two_faces"] == 0 and un["index_out_of_range"] == 0
