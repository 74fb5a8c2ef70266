"""The tiling laws of tests/mesh_tiling.py, proven without a GPU: for K = 2 and 3 every expected_* function, fed the restatement's result
on the base, is compared byte for byte with the restatement run on the tiled mesh itself -- every stage and every base that
tests/test_gpu_mesh_large.py uses, the padded and the copy-interleaved forms included.  The kernels are not involved: what passes here is
that the expectation the GPU is held to at 2^18 vertices is the restatement's own answer.

Left out of the tiling, and why:
  the decimation's selection round and whole call.  A round ranks all costs together and lets the lowest ceil(need / 2) ranks take part;
  equal costs in different copies are ranked by key, so the budget is spent on copy 0 first and the result is not the base's repeated
  (test_decimation_round_is_not_the_bases_repeated shows it on the height field).  meshdecimate_restatement is vectorised.  Measured on
  the 595-fold height field (262395 vertices, 476000 faces, 1428000 table entries), one CPU core: quadrics 3.4 s, the cost entries 18 s,
  one round 16 - 21 s (18 of them the cost entries again), the whole call to 90 % of the faces 62 s in 4 rounds, and a round more for
  every further tenth.  So the GPU tests hold ONE round to the restatement directly, on the smallest mesh that is past the merge sort
  (437-fold, 13 s), and the whole call stays with its small meshes: a target that takes more than a few rounds is minutes of CPU.
  The quadrics and the cost entries are local and are in."""
import numpy as np
import pytest

import mesh_tiling as tl
import meshclean_restatement as mr
import meshclose_restatement as mc
import meshdecimate_restatement as md
import meshfill_restatement as mf
import meshstitch_restatement as ms_
import meshsubdivide_restatement as ms
import meshtrim_restatement as mt

KS = (2, 3)
CLEAN = ("height_field", "book_in_grid_65", "cut_plane", "pieces")
TRIM = ("height_field", "book_in_grid_65")
CLOSE = ("cut_plane", "annulus_16", "book_in_grid_65")
DECIMATE = ("height_field", "messy", "book_in_grid_65")
SUBDIVIDE = ("height_field", "patterns", "book_in_grid_65", "cut_plane", "layered")
SOLVE = ("height_field", "book_in_grid_65")


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---- the tiling itself -----------------------------------------------------------------------------------------------------------------------
def test_tile_shifts_indices_and_keeps_coordinates():
    v, f = tl.base("cut_plane")
    V, F = tl.tile(v, f, 3, pad=5)
    assert V.dtype == np.float32 and F.dtype == np.int32 and len(V) == 3 * len(v) + 5 and len(F) == 3 * len(f)
    for c in range(3):
        assert same(V[c * len(v):(c + 1) * len(v)], v) and np.array_equal(F[c * len(f):(c + 1) * len(f)], f + c * len(v))
    assert (V[3 * len(v):] == v[0]).all() and F.max() < 3 * len(v)
    assert same(V.min(0), v.min(0)) and same(V.max(0), v.max(0))                  # the box of all vertices is the base's
    Vi, Fi = tl.tile(v, f, 3, interleave=True)
    assert same(Vi, V[:3 * len(v)]) and all(np.array_equal(Fi[c::3], f + c * len(v)) for c in range(3))


def test_boundary_counts_lie_either_side():
    for name in ("height_field", "book_in_grid_65", "patterns", "cut_plane", "messy"):
        v, f = tl.base(name)
        k = tl.boundary_counts(len(v), len(f))
        assert k["faces_below"] * len(f) < tl.BOUNDARY < k["faces_above"] * len(f) and k["faces_above"] - k["faces_below"] <= 2
        assert k["vertices_below"] * len(v) < tl.BOUNDARY < k["vertices_above"] * len(v)
        assert 3 * k["entries_below"] * len(f) <= tl.MERGE_SORT_LIMIT < 3 * k["entries_above"] * len(f) and k["entries_above"] == k["entries_below"] + 1


# ---- clean -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", CLEAN)
def test_clean_laws(name, K):
    v, f = tl.base(name)
    V, F = tl.tile(v, f, K)
    for il in (False, True):
        lab, n = tl.expected_components(mr.components(f), len(f), K, il)
        wl, wn = mr.components(tl.tile(v, f, K, interleave=il)[1])
        assert n == wn and same(lab, wl)
    border = int(mr.incidences(f, len(v))[1].sum())
    for steps, cot, bnd in ((1, True, True), (3, False, True), (2, True, False)):
        got, nb = tl.expected_smooth(mr.smooth(v, f, steps, cot, bnd), K, border)
        assert same(got, mr.smooth(V, F, steps, cot, bnd)) and nb == int(mr.incidences(F, len(V))[1].sum())
    removed = 0
    for kw in (dict(smooth_steps=0), dict(smooth_steps=1), dict(smooth_steps=0, min_piece=0.5), dict(smooth_steps=0, min_piece=0.01),
               dict(smooth_steps=0, min_piece=2.0, relative=False)):
        base = mr.clean(v, f, **kw)
        removed += 0 < base[2]["components_removed"] < base[2]["components"]
        ev, ef, est = tl.expected_clean(base, K)
        wv, wf, wst = mr.clean(V, F, **kw)
        assert same(ev, wv) and same(ef, wf) and est == wst, (kw, est, wst)
    assert removed or name != "pieces"                                            # the relative threshold took some pieces and left others


# ---- trim --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", TRIM)
def test_trim_laws(name, K):
    v, f = tl.base(name)
    V, F = tl.tile(v, f, K)
    x = tl.smooth_values(len(v))
    for steps in (1, 5):
        assert same(tl.expected_value_smooth(mt.value_smooth(x, f, steps), K), mt.value_smooth(np.tile(x, K), F, steps))
    x = tl.trim_values(len(v))
    moved = 0
    for ratio in (0.0, 0.01, 0.3):
        base = mt.split(v, f, x, 7.0, ratio)
        want = mt.split(V, F, np.tile(x, K), 7.0, tl.split_ratio(base, ratio, K))
        got = tl.expected_split(base, len(v), len(f), K)
        for k in ("vertices", "faces", "src", "side", "label"):
            assert same(got[k], want[k]), (ratio, k)
        assert got["stats"] == want["stats"] and got["D2"] == want["D2"]
        moved += base["stats"]["moved_to_dropped"] + base["stats"]["moved_to_kept"]
    assert moved > 0                                                              # the ratio that was passed decided something


# ---- close -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", CLOSE)
def test_close_laws(name, K):
    v, f = tl.base(name)
    V, F = tl.tile(v, f, K)
    want = mc.border_loops(F, len(V))
    label, size, nc = tl.expected_border_loops(mc.border_loops(f, len(v)), len(f), K)
    assert same(label, want["label"]) and same(size, want["size"]) and nc == len(want["components"])
    for max_hole in (5, 30, 64):
        ef, est = tl.expected_close_holes(mc.close_holes(v, f, max_hole), len(v), len(f), K)
        wv, wf, wst, _ = mc.close_holes(V, F, max_hole)
        assert same(ef, wf) and est == wst and same(wv, V)


# ---- decimate: the local entries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", DECIMATE)
def test_decimation_quadrics_and_costs_laws(name, K):
    v, f = tl.base(name)
    V, F = tl.tile(v, f, K)
    for bw in (1.0, 4.0):
        assert same(tl.expected_quadrics(md.quadrics(v, f, bw), K), md.quadrics(V, F, bw))
    Vp, Fp = tl.tile(v, f, K, pad=3)
    assert same(tl.expected_quadrics(md.quadrics(v, f), K, pad=3), md.quadrics(Vp, Fp))
    Q = md.quadrics(v, f)
    got = tl.expected_costs(md.collapse_costs(v, f, Q, md.params()), len(v), K)
    want = md.collapse_costs(V, F, tl.expected_quadrics(Q, K), md.params())[:5]
    for g, w, what in zip(got, want, ("key", "multiplicity", "cost", "reject", "position")):
        assert same(g, w), what


def test_decimation_round_is_not_the_bases_repeated():
    v, f = tl.base("height_field")
    Q = md.quadrics(v, f)
    one = md.collapse_round(v, f, Q, 1, md.params())
    V, F = tl.tile(v, f, 2)
    two = md.collapse_round(V, F, tl.expected_quadrics(Q, 2), 2, md.params())      # need 1 a copy: a budget of ceil(2 / 2) = 1 rank for both
    assert one["kept"] == 1 and two["kept"] == 1
    kept_in = [int(((two["selected"][:two["kept"]] >> np.uint64(32)) // np.uint64(len(v)) == c).sum()) for c in range(2)]
    assert kept_in == [1, 0]                                                      # copy 0's edge ranks first by key and takes it: not the base's choice twice


# ---- subdivide ---------------------------------------------------------------------------------------------------------------------------------
def _thresholds(name, v):
    if name == "patterns":
        return (dict(threshold=ms.PATTERN_THR),)
    return (dict(), dict(threshold_fraction=tl.ADAPTIVE_FRACTION.get(name, 0.04)))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SUBDIVIDE)
def test_subdivision_laws(name, K):
    v, f = tl.base(name)
    some = False
    for kw in _thresholds(name, v):
        thr = ms.threshold_of(v, kw.get("threshold", 0.0), kw.get("threshold_fraction", 0.0))
        w = ms.loop_step(v, f, thr)
        stats = ms.subdivide(v, f, iterations=1, **kw)[2]
        some |= 0 < w["n_split"] < len(w["keys"])
        for pad, il in ((0, False), (4, False), (0, True), (4, True)):
            V, F = tl.tile(v, f, K, pad, il)
            assert ms.threshold_of(V, kw.get("threshold", 0.0), kw.get("threshold_fraction", 0.0)) == thr
            W = ms.loop_step(V, F, thr)
            got = tl.expected_subdivide_stage(w, v, K, pad)
            for k in ("keys", "multiplicity", "split", "odd", "vertex_class", "even"):
                assert same(got[k], W[k]), (kw, pad, il, k)
            ev, ef, est = tl.expected_subdivide(w, stats, v, f, K, pad, il)
            wv, wf, wst = ms.subdivide(V, F, iterations=1, **kw)
            assert same(ev, wv) and same(ef, wf) and est == wst, (kw, pad, il, est, wst)
    assert some or name == "layered"                                              # an adaptive case split some edges and left others


def test_subdivision_that_splits_nothing():
    v, f = tl.base("cut_plane")
    w, stats = ms.loop_step(v, f, 100.0), ms.subdivide(v, f, iterations=1, threshold=100.0)[2]
    V, F = tl.tile(v, f, 3, 2)
    ev, ef, est = tl.expected_subdivide(w, stats, v, f, 3, 2)
    wv, wf, wst = ms.subdivide(V, F, iterations=1, threshold=100.0)
    assert stats["iterations"] == 0 and same(ev, wv) and same(ef, wf) and est == wst


# ---- the solve stages --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SOLVE)
def test_solve_laws(name, K):
    v, f = tl.base(name)
    V, F = tl.tile(v, f, K)
    best, c, G = tl.colouring(len(v))
    for steps in (1, 20):
        x, rel = ms_.solve(f, best, c, G, 0.01, steps)
        X, REL = ms_.solve(F, np.tile(best, K), np.tile(c, (K, 1)), np.tile(G, (K, 1)), 0.01, steps)
        assert same(tl.expected_solve(x, K), X) and abs(REL - rel) <= 1e-9 * rel
    x0, level, L = mf.front(f, c, best)
    assert L >= 1
    for steps in (1, 20):
        x = mf.solve(f, x0, level, L, steps)
        assert same(tl.expected_solve(x, K), mf.solve(F, np.tile(x0, (K, 1)), np.tile(level, K), L, steps))


# ---- the globals decided by two outliers behind the last copy ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_outlier_laws(K):
    v, f = tl.base("height_field")
    pad = 3
    V2, F, out = tl.with_outliers(v, f, K, pad)
    thr = ms.threshold_of(V2, 0.0, 0.04)
    assert thr > ms.threshold_of(v, 0.0, 0.04)
    w, stats = ms.loop_step(v, f, thr), ms.subdivide(v, f, iterations=1, threshold=thr)[2]
    ev, ef, est = tl.expected_subdivide(w, stats, v, f, K, pad + 2)
    ev[K * len(v) + pad:K * len(v) + pad + 2] = out
    wv, wf, wst = ms.subdivide(V2, F, iterations=1, threshold_fraction=0.04)
    assert same(ev, wv) and same(ef, wf) and est == wst
    x = tl.trim_values(len(v))
    X = np.concatenate([np.tile(x, K), np.full(pad, x[0]), [7.0 - 50.0, 7.0 + 50.0]])
    got, want = tl.expected_split(mt.split(v, f, x, 7.0, 0.0), len(v), len(f), K), mt.split(V2, F, X, 7.0, 0.0)
    assert same(got["vertices"], want["vertices"]) and same(got["faces"], want["faces"]) and same(got["label"], want["label"])
    assert want["D2"] > got["D2"] and want["stats"]["cut_edges"] == got["stats"]["cut_edges"]
    v, f = tl.base("pieces")
    V2, F, out = tl.with_outliers(v, f, K, pad)
    D = float(mr.box_diameter(V2.min(0), V2.max(0))[0])
    ev, ef, est = tl.expected_clean(mr.clean(v, f, smooth_steps=0, min_piece=0.01 * D, relative=False), K)
    est.update(diameter=D, threshold=0.01 * D, n_vertices_in=len(V2), vertices_dropped=est["vertices_dropped"] + pad + 2)
    wv, wf, wst = mr.clean(V2, F, smooth_steps=0, min_piece=0.01)
    assert same(ev, wv) and same(ef, wf) and est == wst and 0 < wst["components_removed"] < wst["components"]


# ---- the hub that grows past 4096 faces in the middle of a call ----------------------------------------------------------------------------------
def test_growing_hub_passes_4096_in_its_second_iteration():
    v, f = tl.growing_hub()
    one = ms.loop_step(v, f, tl.GROWING_THR)
    assert one["max_valence"] == 2060 and one["vertex_class"][0] == ms.V_INTERIOR and one["even"][0].tobytes() == v[0].tobytes()
    two = ms.loop_step(one["V"], one["F"], tl.GROWING_THR)
    assert two["max_valence"] == 4120 > 4096 and two["vertex_class"][0] == ms.V_INTERIOR
    assert two["even"][0].tobytes() != one["V"][0].tobytes()                       # vertex 0 moves in iteration 2: beta_4120 is read
    st = ms.subdivide(v, f, iterations=2, threshold=tl.GROWING_THR)[2]
    assert st["iterations"] == 2 and st["max_valence"] == 4120
