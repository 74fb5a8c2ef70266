"""The unfriendly-topology fixtures (tests/mesh_topology_fixtures.py) and the mesh stages' numpy restatements, without a GPU: that each
fixture reaches the run lengths, block straddles and boundaries it is for, and that the restatements -- the expected values of
tests/test_gpu_mesh_topology.py -- agree on these meshes with definitions that share no code with them: scipy's connected components, a
dict of edges, Python sets, exact rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import mesh_topology_fixtures as tf
import meshclean_restatement as mr
import meshclose_restatement as mc
import meshdecimate_restatement as md
import meshtrim_restatement as mt


def distinct(t):
    return t[0] != t[1] and t[1] != t[2] and t[0] != t[2]


def edges_of(f):
    """{(lo, hi): [faces, ascending, one entry per incidence]} over the faces with three distinct indices"""
    e = {}
    for i, t in enumerate(np.asarray(f).tolist()):
        if distinct(t):
            for j in range(3):
                a, b = t[j], t[(j + 1) % 3]
                e.setdefault((min(a, b), max(a, b)), []).append(i)
    return e


# ---- 1: the fixtures reach what they are for ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,closed", [(n, c) for n in tf.HUB_SIZES for c in (False, True)] + [(1000, False)])
def test_hub_valence_and_where_its_list_lies(n, closed):
    v, f = tf.hub(n, closed)
    assert v.dtype == np.float32 and f.dtype == np.int32 and len(v) == n + 1 + closed and len(f) == n * (1 + closed)
    assert (f == 0).any(1).sum() == n and (not closed or (f == n + 1).any(1).sum() == n)
    sp = tf.sorted_positions(f, len(v))
    s, e = sp.list(0)
    assert (s, e) == (0, n) and tf.straddles(s, e, 64) == (n > 64) and tf.straddles(s, e, 256) == (n > 256)
    if closed:
        s, e = sp.list(n + 1)
        assert e - s == n and e == 3 * len(f) and (n <= 64 or tf.straddles(s, e, 64)) and (n <= 256 or tf.straddles(s, e, 256))
    inc = {k: len(x) for k, x in edges_of(f).items()}
    assert set(inc.values()) == ({2} if closed else {1, 2}) and sum(1 for c in inc.values() if c == 1) == (0 if closed else n)
    assert sp.longest_run() == 2
    assert np.linalg.matrix_rank(v[1:n + 1].astype(np.float64) - v[1].astype(np.float64)) == 3          # the rim is not planar


@pytest.mark.parametrize("n", tf.BOOK_SIZES)
def test_book_run_length_straddles_and_distant_duplicates(n):
    for d in (0, 2):
        v, f = tf.book(n, duplicates=d)
        assert len(v) == n + 2 and len(f) == n + d
        sp = tf.sorted_positions(f, len(v))
        s, e = sp.run(0, 1)
        assert (s, e) == (0, n + d) and sp.longest_run() == n + d
        assert tf.straddles(s, e, 64) == (n + d > 64) and tf.straddles(s, e, 256) == (n + d > 256)
        assert (sp.edge_val[s:e] // 3).tolist() == list(range(n + d))                                      # the faces of a run ascend
        for k in range(d):
            assert sorted(f[n + k].tolist()) == sorted(f[k].tolist()) and f[n + k].tolist() != f[k].tolist()
            at = (sp.edge_val[s:e] // 3).tolist()
            assert at.index(n + k) - at.index(k) == n and (n < 256 or at.index(n + k) - at.index(k) >= 256)
        if d:
            rev = lambda t: [t[0], t[2], t[1]]
            cyc = lambda t: [t[t.index(min(t)):] + t[:t.index(min(t))]][0]
            assert cyc(f[n].tolist()) == cyc(f[0].tolist()) and cyc(f[n + 1].tolist()) == cyc(rev(f[1].tolist()))    # one as it is, one reversed
        # both spine vertices' corner lists are as long as the run
        assert sp.list(0) == (0, n + d) and sp.list(1) == (n + d, 2 * (n + d))
    wound = [t[:2] for t in tf.book(n)[1].tolist()]
    assert wound == [[0, 1] if i % 2 == 0 else [1, 0] for i in range(n)]
    assert [t[:2] for t in tf.book(n, sides=np.ones(n))[1].tolist()] == [[1, 0]] * n


@pytest.mark.parametrize("n", [65, 257])
def test_book_in_grid_run_is_interleaved_with_an_ordinary_mesh(n):
    v, f = tf.book_in_grid(n)
    a, b = tf.SPINE_IN_GRID
    assert len(v) == 144 + n and len(f) == 242 + n
    e = edges_of(f)
    assert len(e[(a, b)]) == n + 2 and sorted(len(x) for k, x in e.items() if k != (a, b))[-1] == 2
    pages = tf.book_in_grid_pages(n)
    assert sorted(set(e[(a, b)]) - set(pages.tolist())) == sorted(i for i, t in enumerate(f.tolist()) if a in t and b in t and max(t) < 144)
    assert (np.diff(pages) >= 1).all() and pages[0] == 0 and pages[-1] > len(f) - 6 and (f[pages] >= 144).any(1).all()
    assert not (f[np.setdiff1d(np.arange(len(f)), pages)] >= 144).any()
    sp = tf.sorted_positions(f, len(v))
    s, e_ = sp.run(a, b)
    assert e_ - s == n + 2 == sp.longest_run() and tf.straddles(s, e_, 64) and (n < 256 or tf.straddles(s, e_, 256))
    faces_of_run = sp.edge_val[s:e_] // 3
    assert (np.diff(faces_of_run) > 0).all() and faces_of_run[-1] - faces_of_run[0] > len(f) - 6          # far apart in index
    for w in (a, b):
        s, e_ = sp.list(w)
        assert e_ - s == n + 6 and tf.straddles(s, e_, 64)


def test_strip_orders_neighbour_distances_and_border():
    n = 4096
    base = tf.strip(n, "ascending")[1]
    for order in tf.STRIP_ORDERS:
        v, f = tf.strip(n, order)
        o = tf.strip_order(n, order)
        assert len(v) == n + 2 and len(f) == n and np.array_equal(f, base[o]) and sorted(o.tolist()) == list(range(n))
        pos = np.empty(n, np.int64)
        pos[o] = np.arange(n)
        gap = np.abs(np.diff(pos))                                                                          # strip neighbours k, k + 1 in the face array
        if order in ("ascending", "descending"):
            assert (gap == 1).all()
        if order == "even_odd":
            assert (gap[0::2] == 2048).all() and (gap[1::2] == 2047).all()
        if order == "shuffled":
            assert gap.max() > 3500 and np.median(gap) > 800 and not np.array_equal(o, np.arange(n))
        e = edges_of(f)
        assert sum(1 for x in e.values() if len(x) == 1) == n + 2 and max(len(x) for x in e.values()) == 2
        for (a, b), x in e.items():                                                                         # exactly the strip's neighbours share an edge
            assert len(x) == 1 or abs(int(o[x[0]]) - int(o[x[1]])) == 1
    b = mc.border_loops(base, n + 2)
    assert len(b["loops"]) == 1 and len(b["loops"][0]) == n + 2 and b["open"] == []


def test_pieces_boundaries_and_diameters():
    v, f = tf.pieces()
    sizes = tf.PIECE_SIZES
    b = tf.piece_bounds()
    assert b.tolist() == [0, 255, 256, 512, 514, 771, 835, 900, 963, 1263] and len(f) == 1263 and len(v) == 1263 + 2 * len(sizes)
    for p in range(len(sizes)):
        own = np.unique(f[b[p]:b[p + 1]])
        assert len(own) == sizes[p] + 2 and (p == 0 or own.min() == np.unique(f[:b[p]]).max() + 1)          # disjoint, and numbered end to end
    d = tf.piece_diameters(v, f)
    assert np.array_equal(np.argsort(d), np.argsort(sizes)) and (np.diff(np.sort(d)) > 0.2).all() and d.min() > 1.0
    gaps = [np.abs(v[np.unique(f[b[p]:b[p + 1]])][:, None, 0] - v[np.unique(f[b[q]:b[q + 1]])][None, :, 0]).min() for p in range(3) for q in range(p + 1, 4)]
    assert min(gaps) > 500.0


@pytest.mark.parametrize("nv", tf.PADDED_SIZES)
def test_padded_uses_the_last_vertex_and_holds_both_repeated_index_faces(nv):
    bv, bf = tf.book_in_grid(65)
    v, f = tf.padded(bv, bf, nv)
    assert len(v) == nv and len(f) == len(bf) + 2 and np.isfinite(v).all()
    m = len(bf) // 2
    a, b = int(bf[0, 0]), int(bf[0, 1])
    assert f[m].tolist() == [a, a, b] and f[m + 1].tolist() == [nv - 1, nv - 1, nv - 1]
    rest = np.delete(f, [m, m + 1], axis=0)
    at = 2 * len(bf) // 3
    assert rest[at, 1] == nv - 1 and v[nv - 1].tobytes() == bv[bf[at, 1]].tobytes() and (np.delete(rest, at, 0) == np.delete(bf, at, 0)).all()
    assert np.array_equal(rest[at, [0, 2]], bf[at, [0, 2]]) and v[:len(bv)].tobytes() == bv.tobytes()
    used = np.zeros(nv, bool)
    used[f.ravel()] = True
    assert used[nv - 1] and not used[len(bv):nv - 1].any()
    assert len(np.unique(v[len(bv):nv - 1], axis=0)) == nv - 1 - len(bv)                                   # the unreferenced vertices are distinct
    sp = tf.sorted_positions(f, nv)
    assert sp.run_key[-1] == nv << 32 and sp.run_end[-1] - sp.run_start[-1] == 6                           # the sentinel run sorts last ...
    assert sp.list(nv) == (3 * len(f) - 6, 3 * len(f)) and sp.list(nv - 1) == (3 * len(f) - 7, 3 * len(f) - 6)   # ... and so does the sentinel list, behind vertex nv - 1's
    # vertex 0 -- next to which a sentinel cut to the bits of nv - 1 would sort -- has corners on either side of the repeated-index faces
    own = np.nonzero((f == 0).any(1) & mr.distinct(f))[0]
    assert own.min() < m < m + 1 < own.max() and len(own) == 65 + 6
    if nv & (nv - 1) == 0:                                                                                 # nv = 2^k: the sentinel needs a bit more than nv - 1 does
        assert int(nv).bit_length() == int(nv - 1).bit_length() + 1


@pytest.mark.parametrize("nv", [255, 256, 257, 65536])
def test_pillow_hole_must_not_take_its_cheaper_diagonal(nv):
    v, f = tf.pillow(nv)
    assert len(v) == nv and np.isfinite(v).all() and f.tolist() == [[0, 2, 1], [0, 3, 2], [1, 1, 2]]
    b = mc.border_loops(f, nv)
    assert list(b["loops"]) == [1] and b["loops"][1] == [1, 2, 3, 0] and b["open"] == []
    ring = v[b["loops"][1]]
    free, t_free = mc.triangulate(ring)                                                                    # ring positions 0 1 2 3 = vertices 1 2 3 0
    assert t_free.tolist() == [[0, 1, 3], [1, 2, 3]]                                                       # left free, the fill is cut along (2, 0): the mesh's own edge
    _, fo, st, info = mc.close_holes(v, f, 30)
    assert st["loops_closed"] == 1 and fo[3:].tolist() == [[1, 3, 0], [1, 2, 3]] and free < mc.triangulate(ring, [[0, 0, 0, 0], [0, 0, 0, 1]] + [[0] * 4] * 2)[0]
    sp = tf.sorted_positions(f, nv)
    assert sp.run(0, 2) == (1, 3) and sp.run_key[-1] == nv << 32                                           # the key looked up lies at the front, the sentinel run at the back


@pytest.mark.parametrize("nv", [256, 65536])
def test_padded_closed_hub_keeps_its_two_lowest_vertices_interior(nv):
    """vertices 0 and 1, next to which a sentinel cut to the bits of nv - 1 would sort, are interior: a corner list that took the
    repeated-index faces' corners in would change the smoothing there (a border vertex only reads its border edges)"""
    v, f = tf.get("padded_%d_hub_65_closed" % nv)
    border = mr.incidences(f, nv)[1]
    assert len(v) == nv and not border[0] and not border[1] and int(border.sum()) == 4 and f[65].tolist() == [0, 0, 1] and f[66].tolist() == [nv - 1] * 3
    start, corner = mr.corner_lists(f, nv)
    assert start[1] - start[0] == 65 and start[2] - start[1] == 4 and start[nv] - start[nv - 1] == 1


# ---- 2: components against scipy --------------------------------------------------------------------------------------------------------------
def scipy_labels(f):
    f = np.asarray(f)
    nf = len(f)
    ok = np.array([distinct(t) for t in f.tolist()])
    rows, cols = [], []
    for faces in edges_of(f).values():
        rows += faces[:-1]
        cols += faces[1:]
    g = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nf, nf))
    _, lab = connected_components(g, directed=False)
    lowest = np.full(lab.max() + 1, nf)
    np.minimum.at(lowest, lab[ok], np.nonzero(ok)[0])
    out = np.where(ok, lowest[lab], -1)
    return out.astype(np.int32), len(set(out[ok].tolist()))


@pytest.mark.parametrize("name", list(tf.CATALOGUE))
def test_component_labels_are_scipys(name):
    v, f = tf.get(name)
    lab, n = mr.components(f)
    want, wn = scipy_labels(f)
    assert np.array_equal(lab, want) and n == wn
    if name.startswith("strip"):
        assert n == 1 and (lab == 0).all()
    if name == "pieces":
        b = tf.piece_bounds()
        assert n == len(tf.PIECE_SIZES) and all((lab[b[p]:b[p + 1]] == b[p]).all() for p in range(n))
    if name.startswith("book_") and not name.startswith("book_in"):
        assert n == 1 and (lab == 0).all()
    if name.startswith("padded"):
        assert (lab == -1).sum() == 2


# ---- 3: incidences and the clean-up's counts against a dict of edges ----------------------------------------------------------------------------
def collinear(p, q, r):
    """exactly: the cross product of the float32 points' differences is zero in rational arithmetic"""
    u = [Fraction(float(q[k])) - Fraction(float(p[k])) for k in range(3)]
    w = [Fraction(float(r[k])) - Fraction(float(p[k])) for k in range(3)]
    return u[1] * w[2] == u[2] * w[1] and u[2] * w[0] == u[0] * w[2] and u[0] * w[1] == u[1] * w[0]


def brute_clean_counts(v, f):
    """(einc [3 nf], border [nv], removed_duplicate, removed_zero_area, removed_nonmanifold, the surviving faces) by the rules of DESIGN 9 f8
    with no piece removed: of the faces on the same three vertices the lowest stays; then repeated indices and faces without area; then
    every face on an edge that more than two survivors share"""
    faces = np.asarray(f).tolist()
    e = edges_of(f)
    einc = np.zeros(3 * len(faces), np.int64)
    border = np.zeros(len(v), bool)
    for i, t in enumerate(faces):
        if distinct(t):
            for j in range(3):
                k = (min(t[j], t[(j + 1) % 3]), max(t[j], t[(j + 1) % 3]))
                einc[3 * i + j] = len(e[k])
                if len(e[k]) == 1:
                    border[list(k)] = True
    alive = [True] * len(faces)
    seen, dup = set(), 0
    for i, t in enumerate(faces):
        if distinct(t):
            if frozenset(t) in seen:
                alive[i], dup = False, dup + 1
            seen.add(frozenset(t))
    zero = 0
    for i, t in enumerate(faces):
        if alive[i] and (not distinct(t) or collinear(v[t[0]], v[t[1]], v[t[2]])):
            alive[i], zero = False, zero + 1
    e2 = edges_of([t if alive[i] else [0, 0, 0] for i, t in enumerate(faces)])
    bad = {i for x in e2.values() if len(x) > 2 for i in x}
    return einc, border, dup, zero, len(bad), [i for i in range(len(faces)) if alive[i] and i not in bad]


@pytest.mark.parametrize("name", ["hub_65", "hub_257", "hub_257_closed", "hub_1000", "book_3_dup", "book_65_dup", "book_257_dup", "book_300_dup", "book_1000_dup",
                                  "book_in_grid_65", "book_in_grid_257", "padded_256_book_in_grid_65"])
def test_incidences_and_removed_counts_are_a_dict_of_edges(name):
    v, f = tf.get(name)
    einc, border = mr.incidences(f, len(v))
    w_einc, w_border, dup, zero, nonman, left = brute_clean_counts(v, f)
    assert np.array_equal(einc, w_einc) and np.array_equal(border, w_border)
    ov, of, st = mr.clean(v, f, smooth_steps=0)
    assert (st["removed_isolated"], st["removed_duplicate"], st["removed_zero_area"], st["removed_nonmanifold"]) == (0, dup, zero, nonman)
    assert st["n_faces"] == len(left) == len(f) - dup - zero - nonman and st["border_vertices"] == int(w_border.sum())
    used = np.unique(f[left]) if left else np.zeros(0, np.int64)
    assert st["n_vertices"] == len(used) and ov.tobytes() == v[used].tobytes() and np.array_equal(used[of], f[left])
    if name == "book_300_dup":                                                  # the two duplicates go first; the spine still has 300 faces: every page goes
        assert (dup, zero, nonman, st["n_faces"], st["n_vertices"]) == (2, 0, 300, 0, 0)
    if name.startswith("book_in_grid"):
        n = int(name.split("_")[-1])
        assert nonman == n + 2 and st["n_faces"] == 240
    if name.startswith("hub"):
        assert (dup, zero, nonman) == (0, 0, 0) and int(w_border.sum()) == (0 if "closed" in name else int(name.split("_")[1]))


# ---- 4: the link condition against Python sets --------------------------------------------------------------------------------------------------
def set_reject_codes(f, nv):
    """{(lo, hi): the first of rules 1-4 of DESIGN 9 f13 that the edge fails, else 0}: 1 more than two faces; 2 an endpoint of such an edge;
    3 the common neighbours of the ends are not as many as the edge's faces; 4 both ends on the border, the edge not"""
    e = edges_of(f)
    nbr = {}
    for a, b in e:
        nbr.setdefault(a, set()).add(b)
        nbr.setdefault(b, set()).add(a)
    locked = {w for k, x in e.items() if len(x) > 2 for w in k}
    on_border = {w for k, x in e.items() if len(x) == 1 for w in k}
    out = {}
    for (a, b), x in e.items():
        if len(x) > 2:
            out[(a, b)] = 1
        elif a in locked or b in locked:
            out[(a, b)] = 2
        elif len(nbr[a] & nbr[b]) != len(x):
            out[(a, b)] = 3
        elif a in on_border and b in on_border and len(x) != 1:
            out[(a, b)] = 4
        else:
            out[(a, b)] = 0
    return out


@pytest.mark.parametrize("name", ["hub_63", "hub_65", "hub_257", "hub_65_closed", "hub_257_closed", "book_in_grid_65", "padded_256_hub_65_closed"])
def test_collapse_reject_codes_are_the_set_restatements(name):
    v, f = tf.get(name)
    key, mult, cost, reject, pos, _ = md.collapse_costs(v, f, md.quadrics(v, f), md.params())
    want = set_reject_codes(f, len(v))
    assert [(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in key] == sorted(want)
    assert mult.tolist() == [len(edges_of(f)[k]) for k in sorted(want)]
    for k, c in zip(sorted(want), (reject & 15).tolist()):
        assert (c if c <= 4 else 0) == want[k], (k, c, want[k])
    codes = np.bincount(reject & 15, minlength=8)
    if name == "book_in_grid_65":                                               # the spine itself, and every edge at either of its ends but the spine
        a, b = tf.SPINE_IN_GRID
        assert codes[1] == 1 and codes[2] == sum(1 for k in want if (a in k or b in k) and k != (a, b)) == 2 * (65 + 5) and codes[0] > 100
    if name.startswith("hub"):                                                  # a hub passes the link rule at every edge: 2 (or, on the open rim, 1) common neighbours
        assert codes[1] == codes[2] == codes[3] == 0


# ---- 5: border loops ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 257, 1000])
def test_open_hub_border_is_one_loop_of_n_entries(n):
    v, f = tf.hub(n)
    b = mc.border_loops(f, len(v))
    assert b["n_border"] == n and list(b["loops"]) == [1] and b["open"] == [] and len(b["loops"][1]) == n
    assert (b["label"][1::3] == 1).all() and (b["size"][1::3] == n).all() and (b["label"][0::3] == -1).all() and (b["label"][2::3] == -1).all()
    ring = b["loops"][1]                                                        # from the head of entry 1, against the faces: 2, 1, n, n - 1, ...
    assert ring == [2, 1] + list(range(n, 2, -1))
    bc = mc.border_loops(tf.hub(n if n < 1000 else 257, closed=True)[1], n + 2)
    assert bc["n_border"] == 0 and bc["loops"] == {}


@pytest.mark.parametrize("n", tf.BOOK_SIZES)
def test_book_border_components_are_all_open(n):
    v, f = tf.book(n)
    b = mc.border_loops(f, len(v))
    assert b["n_border"] == 2 * n and b["loops"] == {} and len(b["open"]) == n == len(b["components"]) and (b["size"][b["label"] >= 0] == 0).all()
    tail, head = f.ravel(), f[:, [1, 2, 0]].ravel()
    on = b["label"] >= 0
    assert np.array_equal(on.reshape(-1, 3), np.tile([False, True, True], (n, 1)))
    even, odd = (n + 1) // 2, n // 2
    for w, (n_in, n_out) in ((0, (even, odd)), (1, (odd, even))):              # page (0, 1, p): 1 -> p and p -> 0 are border; page (1, 0, p): 0 -> p and p -> 1
        assert (int((head[on] == w).sum()), int((tail[on] == w).sum())) == (n_in, n_out) and n_in + n_out == n
    assert sorted(len(x) for x in b["components"].values()) == [2] * n


# ---- 6: neighbour lists ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("hub_65", 65), ("hub_257", 257), ("hub_257_closed", 257), ("hub_1000", 1000)])
def test_hub_neighbour_list_has_degree_2n_in_corner_order(name, n):
    v, f = tf.get(name)
    start, nbr = mt.neighbours(f, len(v))
    assert start[0] == 0 and start[1] == 2 * n
    assert nbr[:2 * n].tolist() == [w for i in range(n) for w in (1 + i, 1 + (i + 1) % n)]
    if "closed" in name:
        assert start[n + 2] - start[n + 1] == 2 * n and nbr[start[n + 1]:start[n + 2]].tolist() == [w for i in range(n) for w in (1 + (i + 1) % n, 1 + i)]
        assert (np.diff(start)[1:n + 1] == 8).all()
    else:
        assert (np.diff(start)[1:n + 1] == 4).all()
