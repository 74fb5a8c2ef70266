"""The stages of the GPU Poisson surface (csrc/k_poisson.hip) off the noisy sphere: the solver's residual cycle by cycle
against the numpy restatement of the same iteration, the field against the direct (sine-transform) solution, the best-iterate
bookkeeping, the iso-value, the extraction on constructed fields (surface through the lattice's border, every tetrahedron case, chi ==
iso on nodes, nothing to extract), the splat with samples on the grid box's faces and on node centres, and the whole path on a torus,
two spheres and a plate.  The restatement is held to the same conditions without a GPU in tests/test_poisson_cpu.py.

Figures (MI355X; profiles/f11_poisson_stage_tests.log; depth 5 unless stated; 29 tests in 4 s):
  history, GPU        sphere 4.98e-1 3.02e-1 5.68e-2 1.50e-2 5.12e-3 1.37e-3 6.13e-4 1.76e-4 6.16e-5 1.94e-5 6.82e-6 2.61e-6: a factor 0.32 a
                      cycle (random 0.37, three nodes 0.36, sphere at depth 6 0.38); 4e-5 after 10 / 10 / 9 / 11 cycles, as the fp64 restatement
  against fp64        max |GPU / fp64 - 1| over the cycles above 1e-4: 1.6e-4, 2.3e-6, 1.4e-4, depth 6 2.7e-5; the GPU's history equals the
                      restatement's float32 one in every printed digit, so tol = max(1e-3, 10 x float32's deviation) = 1.6e-3, 1e-3, 1.4e-3, 1e-3
  what tol sees       built with the restriction factor 0.25 the GPU's history is off by 58 % .. 2072 %, with the upward sweep in the downward
                      colour order by 43 % .. 281 %; both builds still converge and pass every other solver test
  field               max |chi - exact| / range: GPU 8.6e-6, 1.2e-5, 2.5e-6, depth 6 2.1e-5; the restatement's conjugate gradients at 4e-5 5.5e-5,
                      1.1e-4, 2.5e-5, 3.4e-4; reported against true residual 1.9433e-5 / 1.9425e-5 (sphere)
  float32 floor       sphere: 16 cycles, best 1.04e-6 at cycle 14, then 1.10e-6, 1.47e-6; true residual of the returned chi 7.8e-7, of the last
                      iterate 1.3e-6 -- both within the 5 %-of-4e-5 band, so the band alone does not tell them apart: the bits of chi do
  iso                 |GPU - restatement| 0 (sphere, cap, torus), 4.6e-19 (plate), 8.9e-16 with four invalid rows mixed in; bounds n 2^-52 max|chi|
                      = 3.7e-11, 9.5e-12, 6.7e-11, 6.3e-11 (a lost - 0.5 moves iso by 2.8e-2 .. 6.1, the mean over n for n_valid by 7.3e-4)
  random field        108 577 vertices, 223 630 faces, no coordinate differs; 8 588 edges in one face, all in a boundary plane; 331 151 in two,
                      none in one; every tetrahedron meets each of its 14 mixed cases at least 1 530 times; trim 1 / 3 keeps 29 818 / 200 799 faces
  right-hand side     largest err / bound: plate 0.29 (scale 1.0), 0.94 (1.1), plate_far 0.36, torus 0.996 / 0.990, node centres 0.92
  shapes              torus Euler 0 (14 780 faces, 0.2896 h from the surface at most, as the restatement), two spheres Euler 4 in two pieces
                      (13 128, 0.2914 h), plate at scale 1.0: max (p - o) / h = 32 exactly, 248 edges in one face, all in a boundary plane
  single changes      each of eight one-line changes to k_poisson.hip fails at least one test here (the log's part D names them)"""
import numpy as np
import pytest

import poisson_restatement as pr
from reconstruction_amd.api import POISSON_REL_RESIDUAL
from test_gpu_poisson import check_rhs

pytestmark = pytest.mark.gpu

RHS = [("sphere", 5), ("random", 5), ("corners", 5), ("sphere", 6)]
FIELD_GRID = np.array([pr.FIELD_O[0], pr.FIELD_O[1], pr.FIELD_O[2], pr.FIELD_H])
OPEN_OK = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0)
CLOSED = dict(OPEN_OK, edge_without_opposite=0, edges_not_in_two_faces=0, unused_vertices=0)
_cache = {}      # references, and (stage_chain) GPU results of the one session-scoped ctx, which is why ctx is no part of the key


def same_bits(a, b):
    """(a call, so that a failure shows False: pytest's explanation of two unequal byte strings of this size takes minutes)"""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def solver_ref(kind, depth):
    """b as the library sees it (rounded to float32), the restatement's histories in both precisions, the direct solution"""
    def make():
        b32 = pr.solver_rhs(kind, depth).astype(np.float32)
        b = b32.astype(np.float64)
        return dict(b32=b32, b=b, h64=pr.pcg_history(b, 12, np.float64)[0], h32=pr.pcg_history(b32, 12, np.float32)[0], exact=pr.solve_exact(b))
    return cached(("rhs", kind, depth), make)


def true_residual(b, chi):
    return np.linalg.norm(b - pr.apply_L(chi.astype(np.float64))) / np.linalg.norm(b)


SHAPES = {"sphere": (lambda: pr.sphere_samples(20000), 1.1), "cap": (lambda: pr.sphere_samples(20000, cap=True), 1.1),
          "torus": (lambda: pr.torus_samples(30000), 1.1), "two_spheres": (lambda: pr.two_spheres_samples(20000), 1.1),
          "plate": (lambda: pr.plate_samples(20000), 1.0)}


def shape_ref(name):
    """samples, scale and the restatement's whole reconstruction (solved to 1e-10) at depth 5"""
    def make():
        xyz, nrm = SHAPES[name][0]()
        R = pr.reconstruct(xyz, nrm, 5, scale=SHAPES[name][1])
        R["xyz"], R["nrm"], R["scale"] = xyz, nrm, SHAPES[name][1]
        return R
    return cached(("shape", name), make)


def stage_chain(ctx, name):
    """right-hand side -> solve -> whole call, on one input: (R, grid, chi, vertices, faces, stats)"""
    def make():
        R = shape_ref(name)
        grid, b, occ, _ = ctx.poisson_rhs(R["xyz"], R["nrm"], 5, R["scale"])
        chi = ctx.poisson_solve(b)[0]
        v, f, st = ctx.poisson_mesh(R["xyz"], R["nrm"], 5, scale=R["scale"], trim_cells=0)
        return R, grid, chi, v, f, st
    return cached(("chain", name), make)


# ---- 1: the residual of every cycle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,depth", RHS)
def test_history_follows_the_restatement_cycle_by_cycle(ctx, kind, depth):
    """Conjugate gradients converge with any symmetric positive preconditioner, so `converged` does not see a wrong restriction factor,
    prolongation, boundary term or colour order: they cost cycles.  The residual after every cycle does.  tol is the restatement's own
    float32 against fp64 history over the compared cycles (what float32 rounding alone does), times 10 for the GPU's other fp64
    summation tree, at least 1e-3; cycles below 1e-4 are near the float32 floor, where the two precisions part."""
    S = solver_ref(kind, depth)
    chi, res, cyc, status, hist = ctx.poisson_solve(S["b32"], rel_residual=1e-12, max_cycles=12)
    h64, h32 = S["h64"], S["h32"]
    sel = np.nonzero(h64 >= 1e-4)[0]
    assert len(h64) == 12 and len(h32) == 12 and len(sel) >= 6 and len(hist) > sel.max()
    tol = max(1e-3, 10.0 * np.abs(h32[sel] / h64[sel] - 1.0).max())
    fmt = lambda h: " ".join("%.4e" % x for x in h)
    print("%s depth %d\n  GPU     %s\n  float32 %s\n  fp64    %s" % (kind, depth, fmt(hist), fmt(h32), fmt(h64)))
    dev = np.abs(hist[sel] / h64[sel] - 1.0)
    print("  cycles compared %d, tol %.3e, max |GPU / fp64 - 1| %.3e, residual ratio per cycle %.3f"
          % (len(sel), tol, dev.max(), (h64[sel[-1]] / h64[0]) ** (1.0 / sel[-1])))
    assert (dev <= tol).all()
    n64 = int(np.nonzero(h64 <= POISSON_REL_RESIDUAL)[0][0]) + 1
    _, dres, dcyc, dstatus, _ = ctx.poisson_solve(S["b32"])
    print("  default: GPU %d cycles to %.3e, fp64 restatement %d" % (dcyc, dres, n64))
    assert dstatus == 0 and dres <= POISSON_REL_RESIDUAL and dcyc <= n64 + 1


# ---- 2: the field against the direct solution ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,depth", RHS)
def test_field_against_the_direct_solution(ctx, kind, depth):
    S = solver_ref(kind, depth)
    rng_ = S["exact"].max() - S["exact"].min()
    coarse, _ = pr.solve(S["b"], POISSON_REL_RESIDUAL)
    gap = np.abs(coarse - S["exact"]).max() / rng_
    chi, gres, cyc, status, hist = ctx.poisson_solve(S["b32"])
    fig = np.abs(chi.astype(np.float64) - S["exact"]).max() / rng_
    true = true_residual(S["b"], chi)
    print("%s depth %d: max |chi - exact| / range: restatement's conjugate gradients at %.0e %.3e, GPU (%d cycles) %.3e; residual reported %.4e, "
          "true %.4e" % (kind, depth, POISSON_REL_RESIDUAL, gap, cyc, fig, gres, true))
    assert status == 0 and gres <= POISSON_REL_RESIDUAL
    assert abs(true - gres) <= 0.05 * POISSON_REL_RESIDUAL
    assert fig <= 4.0 * gap


# ---- 3: the best iterate ------------------------------------------------------------------------------------------------------------------
def test_best_iterate_is_what_comes_back(ctx):
    """A target below the float32 floor: the solve ends two cycles after its best one, reports that one's residual and hands back that
    one's chi -- the very bytes a solve stopped at that cycle by max_cycles returns."""
    S = solver_ref("sphere", 5)
    chi, res, cyc, status, hist = ctx.poisson_solve(S["b32"], rel_residual=1e-12, max_cycles=40)
    print("floor: %d cycles, reported %.4e, history tail %s" % (cyc, res, " ".join("%.4e" % x for x in hist[-4:])))
    assert status == 1 and 3 <= cyc < 40 and len(hist) == cyc
    assert res == hist.min() and int(np.argmin(hist)) + 1 == cyc - 2
    true = true_residual(S["b"], chi)
    print("floor: true residual of the returned chi %.4e" % true)
    assert abs(true - res) <= 0.05 * POISSON_REL_RESIDUAL
    chi_b, res_b, cyc_b, status_b, hist_b = ctx.poisson_solve(S["b32"], rel_residual=1e-12, max_cycles=cyc - 2)
    assert cyc_b == cyc - 2 and status_b == 1 and res_b == res and np.array_equal(hist_b, hist[:cyc - 2])
    assert same_bits(chi_b, chi)
    chi1, res1, cyc1, status1, hist1 = ctx.poisson_solve(S["b32"], rel_residual=1e-12, max_cycles=1)
    assert cyc1 == 1 and status1 == 1 and res1 == hist1[0] == hist[0]
    assert abs(true_residual(S["b"], chi1) - res1) <= 0.05 * POISSON_REL_RESIDUAL


def test_zero_and_single_node_right_hand_sides(ctx):
    z = np.zeros((32, 32, 32), np.float32)
    chi, res, cyc, status, hist = ctx.poisson_solve(z)
    assert not chi.any() and status == 0 and cyc == 0 and res == 0.0 and len(hist) == 0
    z[9, 30, 0] = 1.0
    chi, res, cyc, status, hist = ctx.poisson_solve(z)
    exact = pr.solve_exact(z)
    print("unit node: %d cycles to %.3e, max |chi - exact| %.3e" % (cyc, res, np.abs(chi - exact).max()))
    true = true_residual(z.astype(np.float64), chi)
    assert status == 0 and 0 < res <= POISSON_REL_RESIDUAL and abs(true - res) <= 0.05 * POISSON_REL_RESIDUAL
    # chi - exact = L^-1 (residual vector): its 2-norm is at most the true residual ||b|| / the smallest eigenvalue of -L (||b|| = 1)
    assert np.linalg.norm(chi - exact) <= true / pr.laplacian_min_eigenvalue(32)


# ---- 4: the iso-value ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "cap", "torus", "plate"])
def test_iso_value_is_the_mean_of_chi_at_the_valid_samples(ctx, name):
    """Both sides sum n fp64 terms bounded by max |chi| in their own order: each is within (n - 1) 2^-53 n max|chi| of the exact sum, the
    means within n 2^-52 max|chi| of each other."""
    R, grid, chi, v, f, st = stage_chain(ctx, name)
    assert np.array_equal(grid, np.array([R["o"][0], R["o"][1], R["o"][2], R["h"]]))
    n = len(R["p"])
    iso = pr.iso_value(chi, R["p"], R["o"], R["h"])
    bound = n * 2.0 ** -52 * np.abs(chi).max()
    print("%s: iso %.17g, restatement on the GPU's chi %.17g, difference %.3e, bound %.3e" % (name, st["iso"], iso, abs(st["iso"] - iso), bound))
    assert st["n_valid"] == n and abs(st["iso"] - iso) <= bound
    # the stages and the whole path are one computation
    sv, sf = ctx.iso_mesh(chi, st["iso"], grid)
    assert len(f) > 1000 and same_bits(sv, v) and same_bits(sf, f)
    if name == "sphere":
        bad_x = np.array([[np.nan, 0, 0], [1, 2, 3], [np.inf, 0, 0], [5, 5, 5]], np.float32)
        bad_n = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0], [np.nan, 0, 0, 0]], np.float32)
        mx, mn = np.concatenate([bad_x[:2], R["xyz"], bad_x[2:]]), np.concatenate([bad_n[:2], R["nrm"], bad_n[2:]])
        _, _, st2 = ctx.poisson_mesh(mx, mn, 5, trim_cells=0)
        print("%s with 4 invalid rows: iso %.17g, difference %.3e" % (name, st2["iso"], abs(st2["iso"] - iso)))
        assert st2["n_valid"] == n and st2["n_invalid"] == 4 and abs(st2["iso"] - iso) <= bound


# ---- 5: extraction off the sphere ---------------------------------------------------------------------------------------------------------
def field_ref(kind):
    def make():
        chi, iso = pr.lattice_field(kind)
        return (chi, iso) + pr.extract(chi, iso, pr.FIELD_O, pr.FIELD_H)
    return cached(("field", kind), make)


@pytest.mark.parametrize("kind", ["random", "closed", "tie0", "tie1"])
def test_extraction_of_constructed_fields_equals_the_restatement(ctx, kind):
    chi, iso, rv, rf, keys = field_ref(kind)
    v, f = ctx.iso_mesh(chi, iso, FIELD_GRID)
    print("%s: %d vertices, %d faces; coordinates that differ %d" % (kind, len(v), len(f), int((v != rv).sum()) if v.shape == rv.shape else -1))
    assert np.array_equal(f, rf) and same_bits(v, rv)
    if kind == "random":    # the independent conditions, on the GPU's own output
        rep = pr.manifold_report(v, f)
        br = pr.boundary_edge_report(v, f, keys, 32)
        cc = pr.tet_case_counts(chi, iso)
        print("random: %s; cases per tetrahedron min %d" % (br, cc[:, 1:15].min()))
        assert {k: rep[k] for k in OPEN_OK} == OPEN_OK and rep["unused_vertices"] == 0
        assert br["once_in_plane"] > 1000 and br["once_off_plane"] == 0 and br["twice_in_plane"] == 0 and br["more_than_twice"] == 0
        assert len(np.unique(v, axis=0)) == len(v)
        assert pr.orientation_products(v, f, keys, chi, iso, pr.FIELD_O, pr.FIELD_H).min() > 0.0
        assert (cc[:, 1:15] > 0).all()
    if kind == "closed":
        assert {k: v_ for k, v_ in pr.manifold_report(v, f).items() if k != "euler"} == CLOSED


def test_nothing_to_extract_is_an_empty_mesh(ctx):
    chi, iso, _, _, _ = field_ref("random")
    for field, level in ((np.full_like(chi, 0.25), 0.25), (np.full_like(chi, 0.25), 0.0), (chi, float(chi.min()) - 1.0), (chi, float(chi.max()) + 1.0),
                         (chi, float(chi.min()))):
        v, f = ctx.iso_mesh(field, level, FIELD_GRID)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_trim_of_the_random_field(ctx):
    chi, iso, rv, rf, keys = field_ref("random")
    occ = (np.random.default_rng(13).uniform(size=chi.shape) < 0.01).astype(np.uint8)
    last = 0
    for t in (1, 3):
        v, f = ctx.iso_mesh(chi, iso, FIELD_GRID, occ, t)
        ev, ef = pr.trim(rv, rf, occ, pr.FIELD_O, pr.FIELD_H, t)
        print("random field, trim %d: %d of %d faces" % (t, len(ef), len(rf)))
        assert last < len(ef) < len(rf) and np.array_equal(f, ef) and same_bits(v, ev)
        last = len(ef)
    one = np.zeros_like(occ)
    one[31, 0, 17] = 1
    v, f = ctx.iso_mesh(chi, iso, FIELD_GRID, one, 40)         # wider than the grid: everything is kept
    assert np.array_equal(f, rf) and same_bits(v, rv)
    v, f = ctx.iso_mesh(chi, iso, FIELD_GRID, np.zeros_like(occ), 1)
    assert v.shape == (0, 3) and f.shape == (0, 3)


# ---- 6: the right-hand side at the box faces ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", [("plate", 1.0), ("plate", 1.1), ("plate_far", 1.0), ("torus", 1.0), ("torus", 1.1), ("nodes", 1.0)])
def test_rhs_at_the_box_faces_and_on_node_centres(ctx, name, scale):
    """plate_far: the plate's corners and its samples with x < 16, so that the last layer of cells along x holds nothing but the two
    corners on the box's far face: only the cell clamp sets occ there."""
    xyz, nrm = pr.node_centre_samples() if name == "nodes" else SHAPES[name.split("_")[0]][0]()
    if name == "plate_far":
        keep = (np.arange(len(xyz)) < 4) | (xyz[:, 0] < 16.0)
        xyz, nrm = xyz[keep], nrm[keep]
    R = pr.rhs_of(xyz, nrm, 5, scale)
    u = (R["p"] - R["o"]) / R["h"]
    if name == "plate_far":
        assert (u[:, 0] == 32.0).sum() == 2 and ((u[:, 0] >= 28.0) & (u[:, 0] < 32.0)).sum() == 0
        assert R["occ"][16, 6, 31] == 1 and R["occ"][16, 26, 31] == 1 and R["occ"][:, :, 28:].sum() == 2
    if name == "plate" and scale == 1.0:            # the cell clamp and the dropped corners are reached
        assert u.max() == 32.0 and u.min() == 0.0 and (u[:, 2] == 16.0).all()
    if name == "nodes":
        assert u.max() == 32.0 and u.min() == 0.0 and (u[2:] - 0.5 == np.floor(u[2:])).all() and len(u) > 500
    check_rhs(ctx, R, xyz, nrm, 5, scale, "%s scale %.1f" % (name, scale))


# ---- 7: the whole path on other topologies --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,euler,pieces", [("torus", 0, 1), ("two_spheres", 4, 2)])
def test_whole_path_torus_and_two_spheres(ctx, name, euler, pieces):
    R, grid, chi, v, f, st = stage_chain(ctx, name)
    dist = pr.torus_distance if name == "torus" else pr.two_spheres_distance
    rep = pr.manifold_report(v, f)
    g, r = dist(v).max() / st["h"], dist(R["verts"]).max() / R["h"]
    print("%s: %d vertices, %d faces, %d cycles; distance to the surface max %.4f h (restatement %.4f h)" % (name, len(v), len(f), st["cycles"], g, r))
    assert st["converged"] and rep == dict(CLOSED, euler=euler)
    assert ctx.mesh_components(f, len(v))[1] == pieces
    assert g <= 2.0 * r


def test_whole_path_plate_runs_into_the_border(ctx):
    R, grid, chi, v, f, st = stage_chain(ctx, "plate")
    ev, ef, keys = pr.extract(chi, st["iso"], R["o"], R["h"])
    assert np.array_equal(ef, f) and same_bits(ev, v)          # the keys are those of the GPU's vertices
    rep = pr.manifold_report(v, f)
    br = pr.boundary_edge_report(v, f, keys, 32)
    print("plate: %d vertices, %d faces, %s" % (len(v), len(f), br))
    assert {k: rep[k] for k in OPEN_OK} == OPEN_OK
    assert br["once_in_plane"] > 50 and br["once_off_plane"] == 0 and br["more_than_twice"] == 0
