"""The host-only parts of the dense-grid Poisson surface: rsm_write_ply_mesh through a small reader, and the numpy
restatement (tests/poisson_restatement.py) held to the conditions the GPU mesh is held to against it.

Figures of the restatement, solved to 1e-10 (measured with this file's inputs; h = grid spacing):
  sphere (radius 50 around (10, -20, 600), noise 0.05, trim 0)   depth 5, 20 000 samples   depth 6, 80 000 samples
    max radial error of the vertices                              0.289 h                   0.272 h      (mean 0.036 h / 0.031 h)
  cap (samples with n^z < -0.3: 7 129 / 27 989 samples)
    vertices whose own cell holds a sample                        0.713 h                   0.766 h
    vertices within one cell of a sample                          1.769 h                   1.210 h
(An earlier prototype that measured only the crossings of the axis-aligned lattice edges gave 0.09 h / 0.07 h on the sphere; the
tetrahedra's face and body diagonals, along which chi is interpolated over sqrt(2) h and sqrt(3) h, carry the larger figures.)
Bounds asserted on the restatement itself come from the method, not from those figures: on the closed sphere the surface stays within
half a cell of the samples' sphere (the resolution of a lattice of spacing h); on the cap a vertex whose own cell holds a sample lies
within the cell's diagonal sqrt(3) h of that sample, which lies on the sphere up to its noise (5 sigma)."""
import numpy as np
import pytest

import poisson_restatement as pr


def test_write_ply_mesh_round_trips(tmp_path):
    from reconstruction_amd import write_ply_mesh
    rng = np.random.default_rng(3)
    v = rng.normal(size=(57, 3)).astype(np.float32)
    f = rng.integers(0, 57, size=(101, 3)).astype(np.int32)
    path = str(tmp_path / "m.ply")
    write_ply_mesh(path, v, f)
    rv, rf = pr.read_ply_mesh(path)
    assert rv.tobytes() == v.tobytes() and np.array_equal(rf, f)
    hdr = open(path, "rb").read().split(b"end_header\n")[0].decode().splitlines()
    assert hdr[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 57"] and "element face 101" in hdr
    write_ply_mesh(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    rv, rf = pr.read_ply_mesh(path)
    assert rv.shape == (0, 3) and rf.shape == (0, 3)


def test_write_ply_mesh_rejects_bad_arguments(tmp_path):
    import ctypes as C
    from reconstruction_amd import _lib
    lib = _lib.load()
    v = np.zeros((3, 3), np.float32)
    f = np.zeros((1, 3), np.int32)
    vp, fp = v.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p)
    path = str(tmp_path / "x.ply").encode()
    assert lib.rsm_write_ply_mesh(None, vp, 3, fp, 1) == _lib.RSM_E_INVALID
    assert lib.rsm_write_ply_mesh(path, None, 3, fp, 1) == _lib.RSM_E_INVALID
    assert lib.rsm_write_ply_mesh(path, vp, 3, None, 1) == _lib.RSM_E_INVALID
    assert lib.rsm_write_ply_mesh(path, vp, -1, fp, 1) == _lib.RSM_E_INVALID
    assert lib.rsm_write_ply_mesh(str(tmp_path / "no" / "dir.ply").encode(), vp, 3, fp, 1) == _lib.RSM_E_INVALID
    assert lib.rsm_write_ply_mesh(path, vp, 3, fp, 1) == _lib.RSM_OK


def test_the_binding_carries_the_poisson_entry_points():
    from reconstruction_amd import CloudOptimization, Context, _lib
    for name in ("rsm_poisson_mesh", "rsm_poisson_mesh_device", "rsm_poisson_last_mesh", "rsm_poisson_last_mesh_device",
                 "rsm_stage_poisson_rhs", "rsm_stage_poisson_solve", "rsm_stage_iso_mesh", "rsm_write_ply_mesh"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert hasattr(Context, "poisson_mesh") and hasattr(CloudOptimization, "mesh")
    import ctypes as C
    assert C.sizeof(_lib.PoissonParams) == 32     # int, (pad), double, double, int, int


def test_tetrahedron_cases_are_complete_and_consistent():
    """Every case's faces use exactly the crossed edges; complementary cases are each other's mirror image."""
    cases = pr.tet_cases()
    assert cases[0] == [] and cases[15] == []
    for m in range(1, 15):
        crossed = {(u, v) for u in range(4) for v in range(u + 1, 4) if ((m >> u) & 1) != ((m >> v) & 1)}
        used = {e for tri in cases[m] for e in tri}
        assert used == crossed
        assert len(cases[m]) == (1 if len(crossed) == 3 else 2)
        mirror = [(t[0], t[2], t[1]) for t in cases[15 - m]]
        assert sorted(map(sorted, cases[m])) == sorted(map(sorted, mirror))
        # same cyclic orientation reversed: the oriented edge sets are opposite
        half = lambda tris: {(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)}
        inner = lambda tris: {e for e in half(tris) if (e[1], e[0]) in half(tris)}
        assert half(cases[m]) - inner(cases[m]) == {(b, a) for a, b in half(cases[15 - m]) - inner(cases[15 - m])}


@pytest.mark.parametrize("depth,n", [(5, 20000), (6, 80000)])
def test_restatement_sphere_is_a_closed_oriented_manifold_near_the_sphere(depth, n):
    xyz, nrm = pr.sphere_samples(n)
    R = pr.reconstruct(xyz, nrm, depth)
    assert R["residual"] <= 1e-10
    rep = pr.manifold_report(R["verts"], R["faces"])
    print("depth %d: %d vertices, %d faces, %s" % (depth, len(R["verts"]), len(R["faces"]), rep))
    assert rep == dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0, edge_without_opposite=0, edges_not_in_two_faces=0,
                       euler=2, unused_vertices=0)
    assert len(np.unique(R["keys"])) == len(R["keys"]) == len(R["verts"])
    assert pr.face_orientation_min(R["verts"], R["faces"]) > 0.0
    err = pr.radial_error_h(R["verts"], R["h"])
    print("depth %d: radial error max %.3f h, mean %.3f h" % (depth, err.max(), err.mean()))
    assert err.max() <= 0.5


@pytest.mark.parametrize("depth,n", [(5, 20000), (6, 80000)])
def test_restatement_cap_and_its_trim(depth, n):
    xyz, nrm = pr.sphere_samples(n, cap=True)
    R = pr.reconstruct(xyz, nrm, depth)
    N = 1 << depth
    c = pr.vertex_cells(R["verts"], R["o"], R["h"], N)
    err = pr.radial_error_h(R["verts"], R["h"])
    own = R["occ"][c[:, 2], c[:, 1], c[:, 0]] != 0
    near = pr.dilate(R["occ"], 1)[c[:, 2], c[:, 1], c[:, 0]] != 0
    print("depth %d: %d samples; own-cell max %.3f h, within one cell max %.3f h" % (depth, len(xyz), err[own].max(), err[near].max()))
    assert own.sum() > 1000
    assert err[own].max() <= np.sqrt(3.0) + 5 * 0.05 / R["h"]
    last = None
    for t in (1, 2, 4):
        tv, tf = pr.trim(R["verts"], R["faces"], R["occ"], R["o"], R["h"], t)
        rep = pr.manifold_report(tv, tf)
        assert rep["index_out_of_range"] == 0 and rep["repeated_index"] == 0 and rep["unused_vertices"] == 0
        assert 0 < len(tf) < len(R["faces"]) and (last is None or len(tf) >= last)    # a wider trim keeps more
        last = len(tf)
        # every kept face is a face of the untrimmed mesh, in order
        full = {tuple(map(tuple, R["verts"][f])) for f in R["faces"]}
        assert all(tuple(map(tuple, tv[f])) in full for f in tf[:: max(1, len(tf) // 500)])


def test_restatement_ignores_invalid_samples_and_handles_empty_input():
    xyz, nrm = pr.sphere_samples(20000)
    bad_x = np.array([[np.nan, 0, 0], [1, 2, 3], [np.inf, 0, 0], [5, 5, 5]], np.float32)
    bad_n = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0], [np.nan, 0, 0, 0]], np.float32)
    A = pr.reconstruct(xyz, nrm, 5)
    B = pr.reconstruct(np.concatenate([bad_x[:2], xyz, bad_x[2:]]), np.concatenate([bad_n[:2], nrm, bad_n[2:]]), 5)
    assert np.array_equal(A["verts"], B["verts"]) and np.array_equal(A["faces"], B["faces"])
    E = pr.reconstruct(bad_x, bad_n, 5)
    assert len(E["verts"]) == 0 and len(E["faces"]) == 0
    E = pr.reconstruct(np.tile(xyz[:1], (10, 1)), nrm[:10], 5)
    assert len(E["verts"]) == 0 and len(E["faces"]) == 0


# ---- the restatement held to what tests/test_gpu_poisson_stages.py then asks of the GPU ---------------------------------------------------
OPEN_OK = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0)
RHS_KINDS = ["sphere", "random", "corners"]


@pytest.mark.parametrize("kind", RHS_KINDS)
def test_direct_solution_solves_and_agrees_with_conjugate_gradients(kind):
    b = pr.solver_rhs(kind)
    x = pr.solve_exact(b)
    res = np.linalg.norm(b - pr.apply_L(x)) / np.linalg.norm(b)
    cg, _ = pr.solve(b, 1e-10)
    gap = np.abs(cg - x).max() / (x.max() - x.min())
    print("%s: direct solution residual %.2e, against conjugate gradients at 1e-10: %.2e of range" % (kind, res, gap))
    assert res < 1e-12 and gap <= 1e-8


def test_vcycle_is_a_symmetric_operator():
    rng = np.random.default_rng(5)
    r1, r2 = rng.normal(size=(16, 16, 16)), rng.normal(size=(16, 16, 16))
    a, b = np.vdot(pr.vcycle(r1), r2), np.vdot(r1, pr.vcycle(r2))
    print("<M r1, r2> = %.15e, <r1, M r2> = %.15e" % (a, b))
    assert abs(a - b) <= 1e-12 * abs(a)
    assert np.vdot(pr.vcycle(r1), r1) < 0.0         # and, like L, negative


@pytest.mark.parametrize("kind", RHS_KINDS)
def test_preconditioned_history_falls_monotonically_to_the_default(kind):
    """The error bound: chi - chi_exact = L^-1 (L chi - b), and ||L^-1|| is 1 / the smallest eigenvalue of -L."""
    b = pr.solver_rhs(kind)
    hist, chi = pr.pcg_history(b, 14, np.float64, stop=4e-5)
    print("%s: fp64 history %s" % (kind, " ".join("%.3e" % v for v in hist)))
    assert hist[-1] <= 4e-5 and len(hist) <= 12 and (np.diff(hist) < 0).all()
    err = np.linalg.norm(chi - pr.solve_exact(b))
    assert err <= hist[-1] * np.linalg.norm(b) / pr.laplacian_min_eigenvalue(b.shape[0])


def check_open_mesh(chi, iso, v, f, keys, orientation):
    """the conditions of an extraction whose surface may run into the lattice's border"""
    N = chi.shape[0]
    rep = pr.manifold_report(v, f)
    assert {k: rep[k] for k in OPEN_OK} == OPEN_OK and rep["unused_vertices"] == 0
    br = pr.boundary_edge_report(v, f, keys, N)
    assert br["once_off_plane"] == 0 and br["twice_in_plane"] == 0 and br["more_than_twice"] == 0
    if orientation:
        assert len(np.unique(v, axis=0)) == len(v)
        assert pr.orientation_products(v, f, keys, chi, iso, pr.FIELD_O, pr.FIELD_H).min() > 0.0
    return rep, br


def test_random_field_extraction_open_border_orientation_and_every_case():
    chi, iso = pr.lattice_field("random")
    v, f, keys = pr.extract(chi, iso, pr.FIELD_O, pr.FIELD_H)
    rep, br = check_open_mesh(chi, iso, v, f, keys, True)
    cc = pr.tet_case_counts(chi, iso)
    print("random field: %d vertices, %d faces, %s; cases per tetrahedron min %d max %d" % (len(v), len(f), br, cc[:, 1:15].min(), cc[:, 1:15].max()))
    assert br["once_in_plane"] > 1000 and br["twice_off_plane"] > 100000
    assert (cc[:, 1:15] > 0).all()
    assert len(f) == (cc * np.array([len(c) for c in pr.tet_cases()])).sum()


def test_closed_random_field_is_closed():
    chi, iso = pr.lattice_field("closed")
    v, f, keys = pr.extract(chi, iso, pr.FIELD_O, pr.FIELD_H)
    rep, br = check_open_mesh(chi, iso, v, f, keys, True)
    assert rep["edge_without_opposite"] == 0 and rep["edges_not_in_two_faces"] == 0 and br["once_in_plane"] == 0


@pytest.mark.parametrize("kind", ["tie0", "tie1"])
def test_ties_keep_the_connectivity(kind):
    """chi == iso on a node is outside, t = 0: every crossed edge of that node puts its vertex on the node.  Connectivity is by lattice
    edge and does not see it; orientation of the slivers is rounding's, not asserted."""
    chi, iso = pr.lattice_field(kind)
    assert (chi == np.float32(iso)).sum() > 1000
    v, f, keys = pr.extract(chi, iso, pr.FIELD_O, pr.FIELD_H)
    check_open_mesh(chi, iso, v, f, keys, False)
    a, b, c = (v[f[:, q]].astype(np.float64) for q in range(3))
    zero = (np.linalg.norm(np.cross(b - a, c - a), axis=1) == 0.0).sum()
    print("%s: %d vertices (%d distinct), %d faces, %d of zero area" % (kind, len(v), len(np.unique(v, axis=0)), len(f), zero))
    assert len(np.unique(v, axis=0)) < len(v) and zero > 0


def test_restatement_torus_two_spheres_and_plate():
    closed = dict(index_out_of_range=0, repeated_index=0, directed_edge_twice=0, edge_without_opposite=0, edges_not_in_two_faces=0,
                  unused_vertices=0)
    R = pr.reconstruct(*pr.torus_samples(30000), 5)
    rep = pr.manifold_report(R["verts"], R["faces"])
    print("torus: %d faces, %s, distance max %.3f h" % (len(R["faces"]), rep, pr.torus_distance(R["verts"]).max() / R["h"]))
    assert rep == dict(closed, euler=0) and pr.components(R["faces"], len(R["verts"])) == 1
    R = pr.reconstruct(*pr.two_spheres_samples(20000), 5)
    rep = pr.manifold_report(R["verts"], R["faces"])
    print("two spheres: %d faces, %s, distance max %.3f h" % (len(R["faces"]), rep, pr.two_spheres_distance(R["verts"]).max() / R["h"]))
    assert rep == dict(closed, euler=4) and pr.components(R["faces"], len(R["verts"])) == 2
    R = pr.reconstruct(*pr.plate_samples(20000), 5, scale=1.0)
    assert ((R["p"] - R["o"]) / R["h"]).max() == 32.0 and ((R["p"] - R["o"]) / R["h"]).min() == 0.0
    rep = pr.manifold_report(R["verts"], R["faces"])
    br = pr.boundary_edge_report(R["verts"], R["faces"], R["keys"], 32)
    print("plate: %d faces, %s" % (len(R["faces"]), br))
    assert {k: rep[k] for k in OPEN_OK} == OPEN_OK
    assert br["once_in_plane"] > 50 and br["once_off_plane"] == 0 and br["more_than_twice"] == 0
