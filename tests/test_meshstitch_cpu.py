"""The numpy restatement of the seam levelling (tests/meshstitch_restatement.py) against independent answers: a direct
sparse solve of the assembled system, the Chebyshev bound, and properties that follow from the definition.  It is the judge of
csrc/k_meshstitch.hip (tests/test_gpu_meshstitch.py), so it is itself tested here, without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import meshcolor_restatement as mr
import meshstitch_restatement as ms
import meshstitch_scenes as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def direct(seed=5):
    """the split plane with true-texture seam differences and its incidences, shared (and left unchanged) by the tests below"""
    if seed not in _cache:
        v, f, tex, best, c = sc.split_plane(seed=seed)
        G, inc = sc.true_texture_G(f, best, tex)
        _cache[seed] = (f, tex, best, c, G, inc)
    return _cache[seed]


# ---- 1: against the direct solve, and the automatic step count ------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.05, 0.01])
def test_chebyshev_meets_its_bound_against_the_direct_solve(lam):
    from scipy.sparse.linalg import spsolve
    f, tex, best, c, G, inc = direct()
    reduction = 1e-4
    assert inc.dmax == 12                                    # an interior vertex of the plane: six edges, each in two faces
    k = ms.auto_steps(lam, inc.dmax, reduction)
    sigma = ms.spectrum(lam, inc.dmax)[2]
    Tk, Tk1 = sc.cheb_closed(sigma, k), sc.cheb_closed(sigma, k - 1)
    print("lambda %g: sigma - 1 = %.6e, k = %d, T_k = %.6e, T_k-1 = %.6e" % (lam, sigma - 1.0, k, Tk, Tk1))
    assert Tk >= (1.0 / reduction) * (1.0 - 1e-12) and Tk1 < (1.0 / reduction) * (1.0 + 1e-12)
    assert k == int(np.ceil(np.arccosh(1.0 / reduction) / sc.acosh1p(sigma - 1.0)))
    x, rel = ms.solve(f, best, c, G, lam, k)
    A, M = ms.assemble(inc, lam)
    cd = c.astype(np.float64)
    b = G + lam * cd
    xs = np.stack([spsolve(A, b[:, ch]) for ch in range(3)], axis=1)
    assert np.abs(A @ xs - b).max() < 1e-9                   # the direct solve is the answer to far below the bound
    for ch in range(3):
        e_k = np.sqrt((M * (x[:, ch] - xs[:, ch]) ** 2).sum())
        e_0 = np.sqrt((M * (cd[:, ch] - xs[:, ch]) ** 2).sum())
        print("  channel %d: ||M^1/2 (x_k - x*)|| = %.4e, reduction * ||M^1/2 (c - x*)|| = %.4e, largest error %.5f levels"
              % (ch, e_k, reduction * e_0, np.abs(x[:, ch] - xs[:, ch]).max()))
        assert e_k <= reduction * e_0 * (1.0 + 1e-9)
    # what it is for: the largest jump across a seam edge against the true texture's own difference
    seam = best[inc.I] != best[inc.J]
    before = np.abs((cd[inc.I] - cd[inc.J]) - (tex[inc.I] - tex[inc.J]))[seam].max()
    after = np.abs((x[inc.I] - x[inc.J]) - (tex[inc.I] - tex[inc.J]))[seam].max()
    print("  largest seam jump %.2f -> %.2f, relative residual %.2e" % (before, after, rel))
    # (a chain whose edges count twice -- the plane's weakest coupling across the seam -- carries the step of 40 over a decay length of
    # sqrt(2 / lam) edges: a slope of 20 sqrt(lam / 2) levels per edge at the seam.  The plane's diagonals only couple it more strongly.)
    assert before == 40.0 and after < 20.0 * np.sqrt(lam / 2.0) and rel < 1e-3


def test_recurrence_and_closed_form_of_T_agree():
    sigma = ms.spectrum(0.01, 12)[2]
    T = ms.cheb_T(sigma, 300)
    for k in (1, 2, 50, 243, 300):
        assert abs(T[k] - sc.cheb_closed(sigma, k)) <= 1e-10 * T[k]
    with pytest.raises(ValueError):
        ms.auto_steps(1e-14, 12, 1e-4)


# ---- 2: no seam, nothing moves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 2, 37, 200])
def test_a_single_view_mesh_comes_back_bit_for_bit(steps):
    f, tex, best, c, G, inc = direct()
    one = np.zeros_like(best)
    G1, deg, counts = ms.rhs(f, c, one)
    assert counts["seam_incidences"] == 0 and counts["incidences"] == deg.sum() == len(inc.I)
    x, rel = ms.solve(f, one, c, G1, 0.01, steps)
    assert x.tobytes() == c.astype(np.float64).tobytes() and rel == 0.0


# ---- 3: the target differences ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam_gradient", [True, False])
def test_G_is_antisymmetric_and_sums_to_zero(seam_gradient):
    import scipy.sparse as sp
    f, best, c, _, marks = sc.planted_plane()
    rng = np.random.default_rng(3)
    V, nv = 3, len(best)
    best = np.where(best >= 0, rng.integers(0, V, nv), -1).astype(np.int32)     # seams everywhere
    vis = rng.random((V, nv)) < 0.6
    col = rng.integers(0, 256, (V, nv, 3)).astype(np.float64)
    inc = ms.Incidences(f, best >= 0)
    g, counts = ms.targets(inc, c.astype(np.float64), best, vis, col, seam_gradient)
    assert (np.abs(g) <= 255.0).all() and (g * 2.0 == np.round(g * 2.0)).all()
    for ch in range(3):
        Gm = sp.coo_matrix((g[:, ch], (inc.I, inc.J)), shape=(nv, nv)).tocsr()  # (duplicates add: an interior edge is there twice)
        assert abs(Gm + Gm.T).max() == 0.0
    G, deg, counts2 = ms.rhs(f, c, best, vis, col, seam_gradient)
    assert counts == counts2 and (G.sum(axis=0) == 0.0).all() and (G[best < 0] == 0.0).all()
    assert counts["seam_incidences"] == counts["seam_two_terms"] + counts["seam_one_term"] + counts["seam_no_term"] > 1000
    if seam_gradient:
        assert min(counts["seam_two_terms"], counts["seam_one_term"], counts["seam_no_term"]) > 100
    else:
        assert counts["seam_no_term"] == counts["seam_incidences"]
    # the incidences themselves: the border once, the inside twice, the fin's edge three times, nothing from a face with a repeated index
    e0, e1 = marks["fin_edge"]
    assert ((inc.I == e0) & (inc.J == e1)).sum() == 3 and ((inc.I == 0) & (inc.J == 1)).sum() == 1 and ((inc.I == 3) & (inc.J == 4)).sum() == 1
    assert ((inc.I == marks["nx"] + 1) & (inc.J == marks["nx"] + 2)).sum() == 2
    assert deg[marks["loose"]] == 0 and deg[marks["lone"]] == 0 and deg[marks["apex"]] == 2 and (deg[best < 0] == 0).all()


# ---- 4: the mean of every component stays -----------------------------------------------------------------------------------------------------
def test_the_mean_of_each_coloured_component_is_kept():
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    f, best, c, _, marks = sc.planted_plane()
    cd = c.astype(np.float64)
    G, deg, counts = ms.rhs(f, c, best, seam_gradient=False)
    reduction, lam = 1e-4, 0.01
    k = ms.auto_steps(lam, int(deg.max()), reduction)
    x, rel, inc = ms.solve(f, best, c, G, lam, k, return_inc=True)
    n, lab = connected_components(sp.coo_matrix((np.ones(len(inc.I)), (inc.I, inc.J)), shape=(len(best),) * 2), directed=False)
    comps = [np.nonzero((lab == l) & (best >= 0))[0] for l in range(n)]
    comps = [m for m in comps if len(m)]
    sizes = sorted(len(m) for m in comps)
    print("components of coloured vertices: %s, %d steps" % (sizes, k))
    assert sizes[:2] == [1, 1] and len(sizes) == 4 and sizes[2] == 12 * 31 + 1           # the lone and the loose vertex, left of the wall (+ apex), right
    for m in comps:
        drift = np.abs((x[m] - cd[m]).mean(axis=0)).max()
        assert drift <= reduction * 255.0, (len(m), drift)
    assert x[marks["lone"]].tobytes() == cd[marks["lone"]].tobytes() and x[marks["loose"]].tobytes() == cd[marks["loose"]].tobytes()
    assert x[best < 0].tobytes() == cd[best < 0].tobytes()
    left = np.arange(len(best)) % marks["nx"] < marks["wall"]
    left[marks["nx"] * marks["ny"]:] = False
    assert np.abs(x - cd)[left & (best >= 0)].max() < 1e-9 and np.abs(x - cd).max() > 10.0  # no seam left of the wall, one right of it


# ---- 5: two constant images -------------------------------------------------------------------------------------------------------------------
def test_two_constant_images_are_levelled_inside_their_range():
    v, f, tex, best, _ = sc.split_plane()
    c = np.where(best[:, None] == 1, 140, 100).astype(np.uint8) * np.ones((1, 3), np.uint8)
    vis = np.ones((2, len(best)), bool)
    col = np.stack([np.full((len(best), 3), 100.0), np.full((len(best), 3), 140.0)])
    G, deg, counts = ms.rhs(f, c, best, vis, col, True)
    assert counts["seam_two_terms"] == counts["seam_incidences"] > 0 and (G == 0.0).all()   # each view's own difference is 0
    x, rel, inc = ms.solve(f, best, c, G, 0.01, ms.auto_steps(0.01, 12, 1e-4), return_inc=True)
    seam = best[inc.I] != best[inc.J]
    jump = np.abs(x[inc.I] - x[inc.J])[seam].max()
    print("largest seam jump 40 -> %.3f; x in [%.6f, %.6f]" % (jump, x.min(), x.max()))
    assert jump < 40.0 / 8.0
    assert x.min() >= 100.0 and x.max() <= 140.0
    row = x[15 * 41:16 * 41, 0]                              # monotone across the seam, and the mean is kept
    assert (np.diff(row) >= -1e-3).all() and abs(x.mean() - c.mean()) <= 1e-4 * 255.0


# ---- 6: the bytes ---------------------------------------------------------------------------------------------------------------------------
def test_bytes_round_half_up_and_clamp():
    x = np.array([[0.5, 1.5, 2.4999999], [254.5, 255.49, 255.5], [-0.5, -0.50001, -3.0], [300.0, 126.5, 127.5], [9.5, 9.5, 9.5]])
    c = np.full((5, 3), 77, np.uint8)
    coloured = np.array([True, True, True, True, False])
    out, clamped = ms.to_bytes(x, c, coloured)
    assert out.tolist() == [[1, 2, 2], [255, 255, 255], [0, 0, 0], [255, 127, 128], [77, 77, 77]]
    assert clamped == 4                                      # 255.5 -> 256, -0.50001 -> -1, -3 and 300; -0.5 -> floor(0) = 0 is no clamp


# ---- 7: the parameter struct ------------------------------------------------------------------------------------------------------------------
def test_stitch_params_layout_as_the_c_compiler_sees_it(tmp_path):
    from reconstruction_amd import _lib
    t, c = "rsm_mesh_stitch_params", _lib.MeshStitchParams
    body = 'printf("%s %%zu\\n", sizeof(%s));\n' % (t, t) + "".join('printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (t, n, t, n) for n, _ in c._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsm.h"\nint main(void) {\n%sprintf("stats %%d\\n", RSM_MESH_STITCH_STATS);\nreturn 0; }\n' % body)
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got[t]) == C.sizeof(c) == 32
    for n, _ in c._fields_:
        assert int(got["%s.%s" % (t, n)]) == getattr(c, n).offset, n
    assert [n for n, _ in c._fields_] == ["lambda", "iterations", "reduction", "seam_gradient"]
    assert int(got["stats"]) == _lib.MESH_STITCH_STATS == 12
    p = c(0.01, 0, 1e-4, 1)
    assert getattr(p, "lambda") == 0.01 and p.reduction == 1e-4 and p.seam_gradient == 1
    for name in ("rsm_mesh_stitch", "rsm_mesh_stitch_device", "rsm_mesh_stitch_last", "rsm_stage_mesh_visibility", "rsm_stage_mesh_stitch_rhs",
                 "rsm_stage_mesh_stitch_solve"):
        assert name in _lib.PROTOTYPES
