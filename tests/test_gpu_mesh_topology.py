"""The mesh units' shared topology layer (csrc/mesh_common.h, csrc/dev_prims.h: the sorted edge table, the corner lists, the union-find, scan
and compaction) off friendly topology: every mesh stage against its numpy restatement on the meshes of tests/mesh_topology_fixtures.py --
one vertex in up to 1000 faces, one edge in up to 1002 faces (runs and lists that cross 64-lane and 256-thread block boundaries in the
sorted tables), strips of 4096 faces in four face orders, pieces that end on 255 / 256 / 257 in face index, and nv = 2^k - 1, 2^k, 2^k + 1
together with repeated-index faces (the sentinel keys nv and nv << 32).  tests/test_mesh_topology_cpu.py asserts what the fixtures reach
and holds the restatements to independent definitions on them.

Everything is exact, by the idiom of each stage's own test file: bytes for float arrays, array_equal for integers, == for the stats.  The one
figure that is a norm over all vertices, the solve stage's relative residual, is held as tests/test_gpu_meshstitch.py holds it.  If bits
differ, look for a contracted multiply-add or another order of a sum; the comparison is not to be loosened.

Not built, because no input reaches it: a run of the split mesh's edge table in which only the first entry is on the last one's side, so
that k_mt_unite walks back through the whole run.  A triangle of the split mesh is on the side of the original vertices it holds, and
every edge of a long run ends in an original vertex, so all the entries of such a run are on one side and each unites with its
predecessor; only the edge between two cut vertices of one face joins both sides, and its run has two entries per face on those three
vertices.  test_split_* cuts through the spine (two runs of n entries, one per half) and beside it (one run of n).

The colour stage's `padded` mesh is the closed hub of 65: the one of 257 has 259 vertices, more than the 256 it is to be padded to.

Two fixtures are there because the kernels, cut on purpose, showed that the others could not notice (profiles/f32_mesh_topology.log).  A
sentinel key cut to the bits of nv - 1 sorts next to vertex 0's keys at nv = 2^k.  In the corner table that puts the repeated-index faces'
corners into the list of vertex 0 or 1: the smoothing of the clean stage reads them only at an interior vertex, and the spine ends of
book_in_grid are border vertices (every page has two border edges), so the clean stage also runs the decimation's padded closed hub, whose
vertices 0 and 1 are interior.  In the edge table it puts the sentinel run in front, which only a search of the table can notice: the
hole fill's look-up of forbidden diagonals, `pillow` -- a hole at vertex 0 whose cheaper diagonal (0, 2) is an edge of the mesh."""
import numpy as np
import pytest

import mesh_topology_fixtures as tf
import meshclean_restatement as mr
import meshclose_restatement as mc
import meshcolor_restatement as mk
import meshdecimate_restatement as md
import meshstitch_restatement as ms
import meshtrim_restatement as mt
from reconstruction_amd import Camera

pytestmark = pytest.mark.gpu

CLEAN = [n for n in tf.CATALOGUE if n != "book_in_grid_65" and not n.startswith("pillow_")]      # (also the decimation's padded hub: its vertices 0 and 1 are interior)
TRIM = ["hub_257", "hub_257_closed", "book_257", "book_300", "book_in_grid_257", "padded_256_book_in_grid_65", "padded_65536_book_in_grid_65"]
CLOSE = ["hub_63", "hub_64", "hub_65", "hub_257", "hub_1000"] + ["book_%d" % n for n in tf.BOOK_SIZES] + [
    "book_in_grid_65", "strip_ascending", "strip_shuffled", "padded_256_book_in_grid_65", "padded_65536_book_in_grid_65"] + tf.names("pillow_")
DECIMATE = ["hub_65", "hub_65_closed", "hub_257", "hub_257_closed", "book_in_grid_65", "book_in_grid_257", "padded_256_hub_65_closed", "padded_65536_hub_65_closed"]
STITCH = ["hub_257", "hub_1000", "book_300", "padded_256_book_in_grid_65", "padded_65536_book_in_grid_65"]
COLOUR = ["hub_257_closed", "book_in_grid_65", "padded_256_hub_65_closed"]
CONTENDED = ["book_1000", "hub_1000", "strip_shuffled"]


def u64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---- 1: clean -- components, smoothing, clean-up, compaction ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLEAN)
def test_component_labels_are_the_restatements_and_the_lowest_face(ctx, name):
    v, f = tf.get(name)
    want, n = mr.components(f)
    got, ng = ctx.mesh_components(f, len(v))
    assert ng == n and np.array_equal(got, want)
    if name.startswith("strip_") or name.startswith(("hub_", "book_")):          # one piece, whatever the order of its faces: the label is face 0
        assert ng == 1 and (got == 0).all()
    if name == "pieces":
        b = tf.piece_bounds()
        assert ng == len(tf.PIECE_SIZES) and all((got[b[p]:b[p + 1]] == b[p]).all() for p in range(ng))
    if name.startswith("padded_"):
        assert (got == -1).sum() == 2 and got[len(f) // 2 - 1] == -1 and got[len(f) // 2] == -1


@pytest.mark.parametrize("name", CLEAN)
def test_smoothing_is_the_restatements_bits(ctx, name):
    v, f = tf.get(name)
    border = int(mr.incidences(f, len(v))[1].sum())
    for steps in (1, 3):
        for cot in (False, True):
            for bnd in (False, True):
                got, nb = ctx.mesh_smooth(v, f, steps, cot, bnd, return_border=True)
                want = mr.smooth(v, f, steps, cot, bnd)
                assert nb == border
                assert got.tobytes() == want.tobytes(), (steps, cot, bnd, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert not np.array_equal(got, v)


@pytest.mark.parametrize("name", CLEAN)
def test_clean_up_is_the_restatements_mesh_and_stats(ctx, name):
    v, f = tf.get(name)
    for steps in (0, 1):
        ov, of, st = ctx.mesh_clean(v, f, smooth_steps=steps)
        wv, wf, wst = mr.clean(v, f, smooth_steps=steps)
        assert np.array_equal(of, wf) and ov.tobytes() == wv.tobytes() and st == wst, (steps, st, wst)
    if name == "book_300_dup":                                                    # the duplicates lie 300 entries behind their originals in the spine's run
        assert (st["removed_duplicate"], st["removed_nonmanifold"], st["n_faces"]) == (2, 300, 0)
    if name == "book_in_grid_257":
        assert (st["removed_nonmanifold"], st["n_faces"]) == (259, 240)
    if name.startswith("padded_"):
        assert st["removed_zero_area"] == 2 and st["vertices_dropped"] >= len(v) - 144 - 65 - 1 and st["n_vertices"] > 60


def test_pieces_go_by_diameter_and_the_rest_is_compacted_across_block_multiples(ctx):
    v, f = tf.get("pieces")
    d = tf.piece_diameters(v, f)
    b = tf.piece_bounds()
    order = np.sort(d)
    for k in range(len(d) - 1):
        t = 0.5 * (order[k] + order[k + 1])                                      # the k + 1 smallest pieces go: in the face array they alternate with the large ones
        ov, of, st = ctx.mesh_clean(v, f, smooth_steps=0, relative=False, min_piece=t)
        wv, wf, wst = mr.clean(v, f, smooth_steps=0, relative=False, min_piece=t)
        assert np.array_equal(of, wf) and ov.tobytes() == wv.tobytes() and st == wst
        gone = d < t
        assert st["components"] == len(d) and st["components_removed"] == k + 1 == int(gone.sum())
        assert st["removed_isolated"] == sum(tf.PIECE_SIZES[p] for p in np.nonzero(gone)[0]) and st["n_faces"] == len(f) - st["removed_isolated"]
        keep = np.concatenate([np.arange(b[p], b[p + 1]) for p in np.nonzero(~gone)[0]])
        used = np.unique(f[keep])
        assert ov.tobytes() == v[used].tobytes() and np.array_equal(used[of], f[keep])


# ---- 2: trim -- value smoothing and the split -----------------------------------------------------------------------------------------------------
def trim_values(nv, spine_cut, seed=8):
    """values round the trim value 7: even vertices above it, odd ones below, so that the cut passes through a hub's star (the rim
    alternates) and through the spine (0, 1), with the pages alternating sides; spine_cut False lifts the spine's end 1 above as well"""
    x = 7.0 + np.where(np.arange(nv) % 2 == 0, 1.0, -1.0) * np.random.default_rng(seed).uniform(0.5, 1.5, nv)
    if not spine_cut:
        x[1] = 7.0 + abs(x[1] - 7.0)
    return x


@pytest.mark.parametrize("name", TRIM)
def test_value_smoothing_is_the_restatements_bits(ctx, name):
    v, f = tf.get(name)
    x = np.random.default_rng(5).normal(7.0, 2.0, size=len(v))
    for steps in (1, 5):
        got, want = ctx.mesh_value_smooth(x, f, steps), mt.value_smooth(x, f, steps)
        assert got.tobytes() == want.tobytes(), (steps, int((got.view(np.uint64) != want.view(np.uint64)).sum()))
    assert not np.array_equal(got, x)


@pytest.mark.parametrize("spine_cut", [True, False])
@pytest.mark.parametrize("name", TRIM)
def test_split_is_the_restatements_mesh_sides_and_labels(ctx, name, spine_cut):
    v, f = tf.get(name)
    x = trim_values(len(v), spine_cut)
    for ratio in (0.0, 0.01):
        want = mt.split(v, f, x, 7.0, ratio)
        ov, of, src, side, label, st = ctx.mesh_split(v, f, x, 7.0, ratio)
        assert ov.tobytes() == want["vertices"].tobytes() and np.array_equal(of, want["faces"])
        assert np.array_equal(src, want["src"]) and np.array_equal(side, want["side"]) and np.array_equal(label, want["label"])
        assert {k: st[k] for k in mt.STAT_KEYS} == want["stats"] and st["diagonal2"] == want["D2"] and st["value_min"] == x.min() and st["value_max"] == x.max()
    assert st["faces_split"] > 60 and st["cut_edges"] > 60
    spine = {"book_257": (0, 1), "book_300": (0, 1), "book_in_grid_257": tf.SPINE_IN_GRID}.get(name)
    if spine:                                                                    # the spine's one cut vertex serves every face on it
        cut = ((spine[0] << 32) | spine[1]) in want["cut_keys"].tolist()
        assert cut == spine_cut


# ---- 3: close -- border loops and the fill ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLOSE)
def test_border_loops_are_the_restatements(ctx, name):
    v, f = tf.get(name)
    want = mc.border_loops(f, len(v))
    label, size, nc = ctx.mesh_border_loops(f, len(v))
    assert np.array_equal(label, want["label"]) and np.array_equal(size, want["size"]) and nc == len(want["components"])
    if name.startswith("hub_"):
        n = int(name.split("_")[1])
        assert nc == 1 and (size[label >= 0] == n).all() and (label >= 0).sum() == n
    if name.startswith("book_") and not name.startswith("book_in"):
        n = int(name.split("_")[1])
        assert nc == n and (size[label >= 0] == 0).all()
    if name.startswith("strip_"):
        assert nc == 1 and (label >= 0).sum() == 4098 and (size[label >= 0] == 4098).all() and label.max() == label[label >= 0].min()


@pytest.mark.parametrize("max_hole", [30, 64])
@pytest.mark.parametrize("name", CLOSE)
def test_close_holes_is_the_restatements_faces_and_stats(ctx, name, max_hole):
    v, f = tf.get(name)
    wv, wf, wst, info = mc.close_holes(v, f, max_hole)
    ov, of, st = ctx.mesh_close_holes(v, f, max_hole)
    assert ov.tobytes() == v.tobytes() == wv.tobytes()
    assert of.dtype == np.int32 and of.shape == wf.shape and of.tobytes() == wf.tobytes()
    assert st == wst
    if name.startswith("hub_"):                                                  # one loop of n entries, closed exactly when n <= max_hole_size
        n = int(name.split("_")[1])
        assert (st["loops"], st["longest_loop"], st["loops_closed"], st["loops_too_long"]) == (1, n, int(n <= max_hole), int(n > max_hole))
        assert len(of) == len(f) + (n - 2 if n <= max_hole else 0)
        if n <= max_hole:
            mc.check_closed(v, f, of, info)
    if name.startswith("pillow_"):                                               # the fill found the mesh's edge (0, 2) in the table and went round it
        assert st["loops_closed"] == 1 and of[3:].tolist() == [[1, 3, 0], [1, 2, 3]]


# ---- 4: decimate -- quadrics, costs, one round, the whole call ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bw", [1.0, 4.0])
@pytest.mark.parametrize("name", DECIMATE)
def test_quadrics_are_the_restatements_bits(ctx, name, bw):
    v, f = tf.get(name)
    assert same_bits(ctx.mesh_quadrics(v, f, bw), md.quadrics(v, f, bw))


_quadrics = {}


def quadrics_of(name):
    if name not in _quadrics:
        _quadrics[name] = md.quadrics(*tf.get(name))
    return _quadrics[name]


@pytest.mark.parametrize("name", DECIMATE)
def test_costs_rejects_and_positions_are_the_restatements(ctx, name):
    v, f = tf.get(name)
    Q = quadrics_of(name)
    want = md.collapse_costs(v, f, Q, md.params())[:5]
    got = ctx.mesh_collapse_costs(v, f, Q)
    for g, w, what in zip(got, want, ("key", "multiplicity", "cost", "reject", "position")):
        assert g.shape == w.shape, what
        assert (u64(g) == u64(w)).all() if what == "cost" else g.tobytes() == np.ascontiguousarray(w, g.dtype).tobytes(), (what, np.nonzero(g != w))
    codes = np.bincount(got[3] & 15, minlength=8)
    if name.startswith("book_in_grid"):
        n = int(name.split("_")[-1])
        assert codes[md.R_NONMANIFOLD] == 1 and got[1].max() == n + 2 and codes[md.R_LOCKED] == 2 * (n + 5)
    assert codes[md.R_OK] > 60


@pytest.mark.parametrize("need", [1, 20, 200])
@pytest.mark.parametrize("name", DECIMATE)
def test_one_round_is_the_restatements(ctx, name, need):
    v, f = tf.get(name)
    Q = quadrics_of(name)
    w = md.collapse_round(v, f, Q, need, md.params())
    gv, gf, gq, gsel, gkept = ctx.mesh_collapse_round(v, f, Q, need)
    assert gf.shape == w["F"].shape and gf.tobytes() == w["F"].tobytes()
    assert gv.tobytes() == w["V"].tobytes() and same_bits(gq, w["Q"])
    assert gsel.tolist() == w["selected"].tolist() and gkept == w["kept"] and gkept >= 1


def test_whole_decimation_of_the_closed_hub_is_the_restatements_bytes(ctx):
    v, f = tf.get("hub_257_closed")
    wv, wf, wst = md.decimate(v, f, md.params(target_faces=100))
    ov, of, st = ctx.mesh_decimate(v, f, target_faces=100)
    assert ov.dtype == np.float32 and of.dtype == np.int32
    assert of.shape == wf.shape and of.tobytes() == wf.tobytes() and ov.shape == wv.shape and ov.tobytes() == wv.tobytes()
    assert {k: st[k] for k in md.STAT_KEYS if k != "max_cost"} == {k: wst[k] for k in md.STAT_KEYS if k != "max_cost"}
    assert u64(st["max_cost"]) == u64(wst["max_cost"])
    assert st["max_valence"] >= 257 and st["rounds"] > 1 and len(of) in (99, 100)


# ---- 5: stitch -- the solve stage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 50])
@pytest.mark.parametrize("name", STITCH)
def test_stitch_solve_is_the_restatement_bit_for_bit(ctx, name, iterations):
    v, f = tf.get(name)
    rng = np.random.default_rng(9)
    best = rng.integers(-1, 2, len(v)).astype(np.int32)
    best[:2] = (0, 1)                                                            # the hub, and both ends of the spine, are coloured
    c = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    G = rng.normal(0.0, 20.0, (len(v), 3))
    want, wrel, inc = ms.solve(f, best, c, G, 0.01, iterations, return_inc=True)
    got, grel = ctx.mesh_stitch_solve(f, best, c, G, 0.01, iterations)
    assert got.tobytes() == want.tobytes(), int((got.view(np.uint64) != want.view(np.uint64)).sum())
    assert abs(grel - wrel) <= 1e-9 * wrel
    assert got[best < 0].tobytes() == c.astype(np.float64)[best < 0].tobytes()
    if name.startswith(("hub_", "book_")):                                       # the hub's (the spine ends') incidences: two per face whose third vertex is coloured too
        n = int(name.split("_")[1])
        assert inc.dmax > n and inc.deg[0] == inc.dmax


# ---- 6: colour ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", COLOUR)
def test_colours_are_the_restatements_in_both_modes(ctx, name):
    v, f = tf.get(name)
    used = np.zeros(len(v), bool)
    used[f[mr.distinct(f)].ravel()] = True
    c = v[used].astype(np.float64).mean(0)
    R = float(np.sqrt(((v[used].astype(np.float64) - c) ** 2).sum(1)).max())
    W, H = 64, 48
    rng = np.random.default_rng(10)
    # two views from above, either side of the mesh, 3 R away, the mesh about 40 pixels across
    cams = [[Camera(camID=k, P=mk.look_at(c + 3.0 * R * np.array(d) / np.linalg.norm(d), c, 60.0, W / 2.0, H / 2.0),
                    image=rng.integers(0, 256, (H, W, 3)).astype(np.uint8), mask=None) for k, d in enumerate(([0.3, 0.4, 1.0], [-0.8, -0.3, 0.6]))]]
    views = mk.views_of(cams)
    e0, e1, ebest, est = mk.color(v, f, views, "both", 0.2, 0.05)
    for mode, want in ((0, e0), (1, e1)):
        rgb, best, st = ctx.mesh_color(v, f, cams, 0.05, mode=mode)
        assert rgb.tobytes() == want.tobytes() and best.tobytes() == ebest.tobytes() and st == est
    assert st["no_normal"] == int((~used).sum()) and (best[~used] == -1).all() and st["coloured"] > 0.2 * used.sum()
    assert set(np.unique(best).tolist()) == {-1, 0, 1}
    if name.startswith("padded_"):
        assert st["no_normal"] == 256 - 67 - 1


# ---- 7: the same bytes twice, where many threads work on one tree -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONTENDED)
def test_contended_union_find_gives_the_same_bytes_twice(ctx, name):
    v, f = tf.get(name)
    a, b = ctx.mesh_components(f, len(v)), ctx.mesh_components(f, len(v))
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] == 1
    p, q = ctx.mesh_border_loops(f, len(v)), ctx.mesh_border_loops(f, len(v))
    assert p[0].tobytes() == q[0].tobytes() and p[1].tobytes() == q[1].tobytes() and p[2] == q[2]
    assert p[2] == {"book_1000": 1000, "hub_1000": 1, "strip_shuffled": 1}[name]
