"""The mesh units (csrc/k_meshclean.hip, k_meshtrim.hip, k_meshclose.hip, k_meshdecimate.hip, k_meshsubdivide.hip, k_meshstitch.hip,
k_meshfill.hip and the topology layer in mesh_common.h / dev_prims.h) past the sizes at which they change path, held exactly: tiled
meshes (tests/mesh_tiling.py) whose expected result is assembled from the numpy restatement's result on the base by laws that
tests/test_mesh_tiling_cpu.py proves against the restatements.  DESIGN.md 9 f43; the run is in profiles/f43_mesh_large.log.

The boundaries, each with the size just below it:
  262144 vertices / faces   a grid capped at 1024 blocks of 256 starts its threads' second trip: k_sd_vertex (writes vclass), k_sd_count
                            (writes fcnt), k_mesh_vertex_box (the box behind min_piece_relative, threshold_fraction and the trim's D2),
                            k_mt_minmax and the reductions on red_grid, k_mst_resid.  `vertices_above` / `faces_above` put the boundary
                            inside the last copy; the padded cases bring the vertex total to 262143 .. 262145 exactly.
  3 nf = 1048576            rocprim's radix_sort_pairs leaves the merge sort (merge_sort_limit) for the onesweep radix sort, the only path that
                            reads sort_pairs' `bits` (32 + key_bits(nv) for the edge table, key_bits(nv) for the corner lists) as digit
                            passes and on whose stability "the faces of a run ascend" rests.  The installed rocprim's onesweep
                            configurations for gfx950 (detail/config/device_radix_sort_onesweep.hpp) sort 8 bits a pass: `layered` at
                            nv = 65535 / 65536 has key_bits(nv) = 16 / 17, so the corner sort is two full passes / two and one bit, the edge
                            sort six full passes / six and one bit -- the sentinel nv << 32 is the only key with that bit.
  interleaved               the faces copy-interleaved: every run and corner list is fed from entries K faces apart.
  4096 faces at a vertex    BETA_ROOM: BetaTable::ensure re-allocates.  Hubs of 4095 / 4096 / 4097 against ms.subdivide itself, the grown table
                            across calls of one context, and a hub that passes 4096 between the two iterations of one call.

Everything is exact by each stage's own idiom: bytes for float arrays, array_equal for integers, == for the stats; the stitch's relative
residual as tests/test_gpu_meshstitch.py holds it.  If bits differ, look for a wrong stride, a sort cut short or another order of a sum;
the comparison is not to be loosened.

Left out: the decimation's whole call (minutes of CPU in the restatement at these sizes) -- one round is held to the restatement
directly, not by tiling: see tests/test_mesh_tiling_cpu.py."""
import numpy as np
import pytest

import mesh_tiling as tl
import mesh_topology_fixtures as tf
import meshclean_restatement as mr
import meshclose_restatement as mc
import meshdecimate_restatement as md
import meshfill_restatement as mf
import meshstitch_restatement as mst
import meshsubdivide_restatement as ms
import meshtrim_restatement as mt

pytestmark = pytest.mark.gpu

ALL = ("faces_below", "faces_above", "vertices_below", "vertices_above", "entries_below", "entries_above")
ABOVE = ("faces_above", "vertices_above", "entries_above")
_tiled, _base = {}, {}


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def cases(*spec):
    """[(base, tag)] for (base, tags) pairs"""
    return [pytest.param(name, tag, id="%s-%s" % (name, tag)) for name, tags in spec for tag in tags]


def count(name, tag):
    v, f = tl.base(name)
    return tl.boundary_counts(len(v), len(f))[tag]


def tiled(name, K, pad=0, interleave=False):
    """the tiled input, built once per module"""
    key = (name, K, pad, interleave)
    if key not in _tiled:
        V, F = tl.tile(*tl.base(name), K, pad, interleave)
        V.setflags(write=False)
        F.setflags(write=False)
        _tiled[key] = (V, F)
    return _tiled[key]


def on_base(what, name, fn, *args):
    """the restatement's result on a base, computed once"""
    key = (what, name) + tuple(repr(a) for a in args)
    if key not in _base:
        _base[key] = fn()
    return _base[key]


def report(stage, name, tag, V, F):
    print("%s %s %s: %d vertices, %d faces, %d table entries" % (stage, name, tag, len(V), len(F), 3 * len(F)))


# ---- 1: clean -- components, smoothing, clean-up with min_piece_relative, compaction ----------------------------------------------------------------
CLEAN = cases(("height_field", ALL), ("book_in_grid_65", ABOVE), ("pieces", ABOVE))


@pytest.mark.parametrize("name,tag", CLEAN)
def test_components(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    want = on_base("components", name, lambda: mr.components(f))
    for il in (False, True) if tag == "entries_above" else (False,):
        V, F = tiled(name, K, 0, il)
        lab, n = tl.expected_components(want, len(f), K, il)
        got, ng = ctx.mesh_components(F, len(V))
        assert ng == n and np.array_equal(got, lab), (il, np.nonzero(got != lab)[0][:8])
    report("components", name, tag, V, F)


@pytest.mark.parametrize("name,tag", CLEAN)
def test_smoothing(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    V, F = tiled(name, K)
    border = int(mr.incidences(f, len(v))[1].sum())
    for steps, cot, bnd in ((1, True, True), (2, False, False)):
        want, nb = tl.expected_smooth(on_base("smooth", name, lambda: mr.smooth(v, f, steps, cot, bnd), steps, cot, bnd), K, border)
        got, gb = ctx.mesh_smooth(V, F, steps, cot, bnd, return_border=True)
        assert gb == nb and got.tobytes() == want.tobytes(), (steps, cot, bnd, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    report("smooth", name, tag, V, F)


@pytest.mark.parametrize("name,tag", CLEAN)
def test_clean_up_with_a_relative_threshold(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    V, F = tiled(name, K)
    # (relative is the default: the threshold is a fraction of the box; 1 % of the pieces' box lies between their diameters)
    for kw in (dict(smooth_steps=1), dict(smooth_steps=0, min_piece=0.01 if name == "pieces" else 0.5)):
        base = on_base("clean", name, lambda: mr.clean(v, f, **kw), sorted(kw.items()))
        wv, wf, wst = tl.expected_clean(base, K)
        ov, of, st = ctx.mesh_clean(V, F, **kw)
        assert st == wst, {k: (st[k], wst[k]) for k in st if st[k] != wst.get(k)}
        assert np.array_equal(of, wf) and ov.tobytes() == wv.tobytes()
        assert st["diameter"] == base[2]["diameter"] and st["threshold"] == base[2]["threshold"]
    if name == "pieces":
        assert 0 < base[2]["components_removed"] < base[2]["components"] and st["components_removed"] == K * base[2]["components_removed"]
    if name == "book_in_grid_65":
        assert base[2]["removed_nonmanifold"] == 67 and st["removed_nonmanifold"] == K * 67
    report("clean", name, tag, V, F)


# ---- 2: density trim -- value smoothing and the split ----------------------------------------------------------------------------------------------------
TRIM = cases(("height_field", ALL), ("book_in_grid_65", ABOVE))


@pytest.mark.parametrize("name,tag", TRIM)
def test_value_smoothing(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    V, F = tiled(name, K)
    x = tl.smooth_values(len(v))
    want = tl.expected_value_smooth(on_base("value_smooth", name, lambda: mt.value_smooth(x, f, 5)), K)
    got = ctx.mesh_value_smooth(np.tile(x, K), F, 5)
    assert got.tobytes() == want.tobytes(), int((got.view(np.uint64) != want.view(np.uint64)).sum())
    report("value_smooth", name, tag, V, F)


@pytest.mark.parametrize("name,tag", TRIM)
def test_split(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    V, F = tiled(name, K)
    x = tl.trim_values(len(v))
    for ratio in (0.0, 0.3):
        base = on_base("split", name, lambda: mt.split(v, f, x, 7.0, ratio), ratio)
        want = tl.expected_split(base, len(v), len(f), K)
        ov, of, src, side, label, st = ctx.mesh_split(V, F, np.tile(x, K), 7.0, tl.split_ratio(base, ratio, K))
        assert {k: st[k] for k in mt.STAT_KEYS} == want["stats"], {k: (st[k], want["stats"][k]) for k in mt.STAT_KEYS if st[k] != want["stats"][k]}
        assert ov.tobytes() == want["vertices"].tobytes() and np.array_equal(of, want["faces"])
        assert np.array_equal(src, want["src"]) and np.array_equal(side, want["side"]) and np.array_equal(label, want["label"])
        assert st["diagonal2"] == want["D2"] and st["value_min"] == x.min() and st["value_max"] == x.max()
    assert st["moved_to_dropped"] + st["moved_to_kept"] > 0 and st["cut_edges"] >= K * 60
    report("split", name, tag, V, F)


# ---- 3: close holes ---------------------------------------------------------------------------------------------------------------------------------
CLOSE = cases(("cut_plane", ALL), ("book_in_grid_65", ABOVE), ("annulus_16", ABOVE))


@pytest.mark.parametrize("name,tag", CLOSE)
def test_border_loops(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    V, F = tiled(name, K)
    wl, ws, wn = tl.expected_border_loops(on_base("border_loops", name, lambda: mc.border_loops(f, len(v))), len(f), K)
    label, size, nc = ctx.mesh_border_loops(F, len(V))
    assert nc == wn and np.array_equal(label, wl) and np.array_equal(size, ws)
    report("border_loops", name, tag, V, F)


@pytest.mark.parametrize("name,tag", CLOSE)
def test_close_holes(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    V, F = tiled(name, K)
    base = on_base("close_holes", name, lambda: mc.close_holes(v, f, 30))
    wf, wst = tl.expected_close_holes(base, len(v), len(f), K)
    ov, of, st = ctx.mesh_close_holes(V, F, 30)
    assert st == wst, {k: (st[k], wst[k]) for k in st if st[k] != wst[k]}
    assert ov.tobytes() == V.tobytes() and of.dtype == np.int32 and of.shape == wf.shape and of.tobytes() == wf.tobytes()
    if name == "cut_plane":
        assert base[2]["loops_closed"] == 3 and st["loops_closed"] == 3 * K
    report("close_holes", name, tag, V, F)


# ---- 4: decimate -- quadrics and costs by tiling, one round against the restatement itself -----------------------------------------------------------------
DECIMATE = cases(("height_field", ALL), ("messy", ABOVE), ("book_in_grid_65", ABOVE))


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("name,tag", DECIMATE)
def test_quadrics_and_costs(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    V, F = tiled(name, K)
    Q = on_base("quadrics", name, lambda: md.quadrics(v, f))
    QK = tl.expected_quadrics(Q, K)
    assert same(ctx.mesh_quadrics(V, F, 1.0), QK)
    want = tl.expected_costs(on_base("costs", name, lambda: md.collapse_costs(v, f, Q, md.params())), len(v), K)
    got = ctx.mesh_collapse_costs(V, F, QK)
    for g, w, what in zip(got, want, ("key", "multiplicity", "cost", "reject", "position")):
        assert g.shape == w.shape, what
        assert (u64(g) == u64(w)).all() if what == "cost" else g.tobytes() == np.ascontiguousarray(w, g.dtype).tobytes(), (what, np.nonzero(g != w)[0][:8])
    assert np.bincount(got[3] & 15, minlength=8)[md.R_OK] >= 10 * K
    report("quadrics_costs", name, tag, V, F)


def test_one_round_past_the_merge_sort_is_the_restatements(ctx):
    """not by tiling (the ranking is global): the restatement runs the tiled mesh itself, about 13 s of CPU"""
    name, tag = "height_field", "entries_above"
    K = count(name, tag)
    V, F = tiled(name, K)
    Q = tl.expected_quadrics(on_base("quadrics", name, lambda: md.quadrics(*tl.base(name))), K)
    need = 2001                                                                   # an odd budget that ends inside a copy's equal costs
    w = md.collapse_round(V, F, Q, need, md.params())
    gv, gf, gq, gsel, gkept = ctx.mesh_collapse_round(V, F, Q, need)
    assert gf.shape == w["F"].shape and gf.tobytes() == w["F"].tobytes()
    assert gv.tobytes() == w["V"].tobytes() and same(gq, w["Q"])
    assert gsel.tolist() == w["selected"].tolist() and gkept == w["kept"] and gkept >= 100
    report("collapse_round", name, tag, V, F)


# ---- 5: subdivide -- the stage entry and the whole call for one iteration -------------------------------------------------------------------------------------
# (base, K, pad, interleave); None: the K of the tag.  The padded cases bring the vertex total to 262144 - 1, + 0, + 1; `layered` to the
# digit boundary of the sorts' passes with 3 nf past the merge sort
def _subdivide_cases():
    out = [(name, tag, count(name, tag), 0, False) for name, tags in (("height_field", ALL), ("patterns", ALL), ("book_in_grid_65", ABOVE), ("cut_plane", ABOVE))
           for tag in tags]
    nv = len(tl.base("height_field")[0])
    K = (tl.BOUNDARY - 1) // nv
    out += [("height_field", "padded_to_%d" % total, K, total - K * nv, False) for total in (tl.BOUNDARY - 1, tl.BOUNDARY, tl.BOUNDARY + 1)]
    out += [("height_field", "interleaved", count("height_field", "entries_above"), 0, True), ("book_in_grid_65", "interleaved", count("book_in_grid_65", "entries_above"), 7, True)]
    nv = len(tl.base("layered")[0])
    K = 65535 // nv
    out += [("layered", "nv_%d" % total, K, total - K * nv, il) for total, il in ((65535, False), (65536, False), (65536, True))]
    return [pytest.param(*c, id="%s-%s%s" % (c[0], c[1], "-interleaved" if c[4] and c[1] != "interleaved" else "")) for c in out]


def _thresholds(name):
    return (dict(threshold=ms.PATTERN_THR),) if name == "patterns" else (dict(), dict(threshold_fraction=tl.ADAPTIVE_FRACTION.get(name, 0.04)))


def _step(name, kw):
    v, f = tl.base(name)

    def run():
        w = ms.loop_step(v, f, ms.threshold_of(v, kw.get("threshold", 0.0), kw.get("threshold_fraction", 0.0)))
        return w, ms.subdivide(v, f, iterations=1, **kw)[2]
    return on_base("loop_step", name, run, sorted(kw.items()))


@pytest.mark.parametrize("name,tag,K,pad,il", _subdivide_cases())
def test_subdivision_stage_entry(ctx, name, tag, K, pad, il):
    v, f = tl.base(name)
    V, F = tiled(name, K, pad, il)
    if name == "layered":
        assert 3 * len(F) > tl.MERGE_SORT_LIMIT and len(V) in (65535, 65536)
    for kw in _thresholds(name):
        w, _ = _step(name, kw)
        want = tl.expected_subdivide_stage(w, v, K, pad)
        got = ctx.mesh_subdivide_edges(V, F, **kw)
        assert got["threshold"] == ms.threshold_of(v, kw.get("threshold", 0.0), kw.get("threshold_fraction", 0.0))
        for k in ("keys", "multiplicity", "split", "odd", "vertex_class", "even"):
            g, e = got[k], want[k]
            assert g.shape == e.shape and g.dtype == e.dtype, (k, g.shape, e.shape, g.dtype, e.dtype)
            assert g.tobytes() == e.tobytes(), (kw, k, np.nonzero(np.atleast_1d((g != e).reshape(len(g), -1).any(1)))[0][:8])
    report("subdivide_edges", name, tag, V, F)


@pytest.mark.parametrize("name,tag,K,pad,il", _subdivide_cases())
def test_subdivision_whole_call_one_iteration(ctx, name, tag, K, pad, il):
    v, f = tl.base(name)
    V, F = tiled(name, K, pad, il)
    for kw in _thresholds(name):
        w, stats = _step(name, kw)
        wv, wf, wst = tl.expected_subdivide(w, stats, v, f, K, pad, il)
        ov, of, st = ctx.mesh_subdivide(V, F, iterations=1, **kw)
        assert st == wst, {k: (st[k], wst[k]) for k in st if st[k] != wst[k]}
        assert ov.dtype == np.float32 and of.dtype == np.int32
        assert of.shape == wf.shape and of.tobytes() == wf.tobytes(), np.nonzero((of != wf).any(1))[0][:8]
        assert ov.shape == wv.shape and ov.tobytes() == wv.tobytes(), np.nonzero((ov != wv).any(1))[0][:8]
        # what comes out of the capped grids' counters: K times the base's, and the base's largest valence
        for k in ("moved_interior", "moved_border", "faces_0_splits", "faces_1_split", "faces_2_splits", "faces_3_splits"):
            assert st[k] == K * stats[k], k
        assert st["locked_vertices"] == K * stats["locked_vertices"] + pad and st["max_valence"] == stats["max_valence"]
    assert st["split_edges"] > 0
    report("subdivide", name, tag, V, F)


# ---- 6: the solve stages of stitch and fill -------------------------------------------------------------------------------------------------------------
SOLVE = cases(("height_field", ALL), ("book_in_grid_65", ABOVE))


@pytest.mark.parametrize("name,tag", SOLVE)
def test_stitch_solve(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    V, F = tiled(name, K)
    best, c, G = tl.colouring(len(v))
    x, rel = on_base("stitch_solve", name, lambda: mst.solve(f, best, c, G, 0.01, 20))
    got, grel = ctx.mesh_stitch_solve(F, np.tile(best, K), np.tile(c, (K, 1)), np.tile(G, (K, 1)), 0.01, 20)
    want = tl.expected_solve(x, K)
    assert got.tobytes() == want.tobytes(), int((got.view(np.uint64) != want.view(np.uint64)).sum())
    assert abs(grel - rel) <= 1e-9 * rel
    report("stitch_solve", name, tag, V, F)


@pytest.mark.parametrize("name,tag", SOLVE)
def test_fill_solve(ctx, name, tag):
    v, f = tl.base(name)
    K = count(name, tag)
    V, F = tiled(name, K)
    best, c, _ = tl.colouring(len(v))

    def run():
        x0, level, L = mf.front(f, c, best)
        return x0, level, L, mf.solve(f, x0, level, L, 20)
    x0, level, L, x = on_base("fill_solve", name, run)
    got = ctx.mesh_fill_solve(F, np.tile(x0, (K, 1)), np.tile(level, K), L, 20)
    want = tl.expected_solve(x, K)
    assert L >= 1 and got.tobytes() == want.tobytes(), int((got.view(np.uint64) != want.view(np.uint64)).sum())
    assert not np.array_equal(x, x0)
    report("fill_solve", name, tag, V, F)


# ---- 7: valence past BETA_ROOM ---------------------------------------------------------------------------------------------------------------------------
def _hub(n, closed):
    return on_base("hub", "%d_%d" % (n, closed), lambda: (tf.hub(n, closed),) + ms.subdivide(*tf.hub(n, closed), iterations=1))


def _same_whole(ctx, v, f, want, **kw):
    wv, wf, wst = want
    ov, of, st = ctx.mesh_subdivide(v, f, **kw)
    assert st == wst, {k: (st[k], wst[k]) for k in st if st[k] != wst[k]}
    assert of.shape == wf.shape and of.tobytes() == wf.tobytes() and ov.shape == wv.shape and ov.tobytes() == wv.tobytes()
    return st


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_a_hub_of_about_4096_faces(ctx, n, closed):
    (v, f), *want = _hub(n, closed)
    st = _same_whole(ctx, v, f, want, iterations=1)
    assert st["max_valence"] == n and st["moved_interior"] >= 1 and want[0][0].tobytes() != v[0].tobytes()      # the hub moved: beta_n was read


def test_the_grown_table_stays_inside_its_call(ctx):
    big, small = _hub(4097, False), _hub(65, False)
    for (v, f), *want in (big, small, big, big, small):
        _same_whole(ctx, v, f, want, iterations=1)


def test_a_hub_that_passes_4096_faces_between_two_iterations(ctx):
    v, f = tl.growing_hub()
    want = on_base("growing_hub", "2060", lambda: ms.subdivide(v, f, iterations=2, threshold=tl.GROWING_THR))
    st = _same_whole(ctx, v, f, want, iterations=2, threshold=tl.GROWING_THR)
    assert st["iterations"] == 2 and st["max_valence"] == 4120
    _same_whole(ctx, *_hub(65, False)[0], _hub(65, False)[1:], iterations=1)


# ---- 8: the globals, decided by vertices of the second trip alone ----------------------------------------------------------------------------------------
# Coincident copies cannot notice a box or an extremum that leaves vertices out: every coordinate occurs K times.  Here the tiled mesh is
# padded to 262144 vertices and two more, unreferenced, lie outside the box (their values outside the values' range): the global is
# theirs alone, and they are vertices 262144 and 262145.  The restatement runs the base with the absolute parameter that follows.
def _with_outliers(name):
    v, f = tl.base(name)
    K = count(name, "vertices_below")
    pad = tl.BOUNDARY - K * len(v)
    V2, F, out = tl.with_outliers(v, f, K, pad)
    assert len(V2) == tl.BOUNDARY + 2 and pad > 0
    return v, f, K, pad, V2, F, out


def test_subdivision_threshold_fraction_reads_the_box_of_the_second_trip(ctx):
    v, f, K, pad, V2, F, out = _with_outliers("height_field")
    thr = ms.threshold_of(V2, 0.0, 0.04)
    assert thr > ms.threshold_of(v, 0.0, 0.04)
    w, stats = ms.loop_step(v, f, thr), ms.subdivide(v, f, iterations=1, threshold=thr)[2]
    assert 0 < w["n_split"] < len(w["keys"])
    wv, wf, wst = tl.expected_subdivide(w, stats, v, f, K, pad + 2)
    wv[K * len(v) + pad:K * len(v) + pad + 2] = out
    ov, of, st = ctx.mesh_subdivide(V2, F, iterations=1, threshold_fraction=0.04)
    assert st["threshold"] == thr and st == wst, {k: (st[k], wst[k]) for k in st if st[k] != wst[k]}
    assert of.tobytes() == wf.tobytes() and ov.tobytes() == wv.tobytes()
    got = ctx.mesh_subdivide_edges(V2, F, threshold_fraction=0.04)
    assert got["threshold"] == thr and np.array_equal(got["split"], np.tile(w["split"], K))


def test_clean_up_relative_threshold_reads_the_box_of_the_second_trip(ctx):
    v, f, K, pad, V2, F, out = _with_outliers("pieces")
    D = float(mr.box_diameter(V2.min(0), V2.max(0))[0])
    assert D > float(mr.box_diameter(v.min(0), v.max(0))[0])
    base = mr.clean(v, f, smooth_steps=0, min_piece=0.01 * D, relative=False)
    wv, wf, wst = tl.expected_clean(base, K)
    wst.update(diameter=D, threshold=0.01 * D, n_vertices_in=len(V2), vertices_dropped=wst["vertices_dropped"] + pad + 2)
    ov, of, st = ctx.mesh_clean(V2, F, smooth_steps=0, min_piece=0.01)
    assert st == wst, {k: (st[k], wst[k]) for k in st if st[k] != wst.get(k)}
    assert np.array_equal(of, wf) and ov.tobytes() == wv.tobytes() and 0 < base[2]["components_removed"] < base[2]["components"]


def test_trim_reads_the_values_and_the_box_of_the_second_trip(ctx):
    v, f, K, pad, V2, F, out = _with_outliers("height_field")
    x = tl.trim_values(len(v))
    X = np.concatenate([np.tile(x, K), np.full(pad, x[0]), [7.0 - 50.0, 7.0 + 50.0]])
    P = V2.astype(np.float64)
    ext = P.max(0) - P.min(0)
    D2 = float((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2])
    ov, of, src, side, label, st = ctx.mesh_split(V2, F, X, 7.0, 0.0)
    assert st["value_min"] == 7.0 - 50.0 and st["value_max"] == 7.0 + 50.0 and st["diagonal2"] == D2
    base = on_base("split", "height_field", lambda: mt.split(v, f, x, 7.0, 0.0), 0.0)
    want = tl.expected_split(base, len(v), len(f), K)                             # (the fixed-point areas are relative to D2: q_total is not the base's)
    assert ov.tobytes() == want["vertices"].tobytes() and np.array_equal(of, want["faces"]) and np.array_equal(label, want["label"])
    assert st["n_vertices_in"] == len(V2) and st["cut_edges"] == want["stats"]["cut_edges"]
