"""Tiled meshes: K copies of a base mesh that are NOT moved -- the same coordinates, vertex indices shifted by c nv, faces copy-major -- and
the law by which each mesh stage's exact result on the tiled mesh follows from its result on the base.  Test infrastructure only, plain
numpy.  The restatements of the mesh stages are partly Python loops and cannot run a mesh of 2^18 vertices; the laws here can, because the
restatement runs once on the base and index arithmetic does the rest.  tests/test_mesh_tiling_cpu.py proves every law at K = 2, 3 against
the restatement run on the tiled mesh itself, byte for byte; tests/test_gpu_mesh_large.py holds the kernels to the laws past the sizes at
which they change path.

Why the laws hold.  Every rule of the mesh units is local to a connected piece (edge runs, corner lists, components, border loops, stars)
or reads a global that coincident copies leave unchanged: the box of all vertices, the extrema of the values, the largest degree.  Copy c's
vertices are c nv .. c nv + nv - 1, so every key (min << 32) | max of copy c lies above all of copy c - 1: the sorted tables are the base's
tables copy after copy, and a run or a corner list of copy c holds copy c's faces in the base's order.  Everything that is numbered in key
order (the new vertices of the subdivision, the cut vertices of the trim) is therefore numbered copy-major within its block, and everything
numbered by face (labels, new faces) is shifted by the faces in front.  Where a global does grow K-fold (the trim's total area), the law
passes the parameter that restores the base's decision and checks that it does.

Options of tile():
  pad         unreferenced vertices appended behind the last copy, at the position of vertex 0 (inside the box, so the box stays): they bring
              a vertex count to a chosen total.  Only the laws that say so take a pad.
  interleave  the faces copy-interleaved instead of copy-major: face i of copy c at position i K + c.  Within a copy the faces keep their
              order, so runs and lists hold the same faces in the same order, but fed from entries K faces apart.

NOT tested by tiling (see the docstring of tests/test_mesh_tiling_cpu.py): the decimation's selection round and whole call.  Equal costs in
different copies are ranked by key under ONE budget of ceil(need / 2) ranks, so copy 0 takes the budget first: the result is not the
base's result repeated.  The restatement of both is vectorised, and the GPU is held to it directly on the tiled mesh."""
from __future__ import annotations

import numpy as np

BOUNDARY = 262144                      # 1024 blocks of 256: a capped grid's second trip starts here
MERGE_SORT_LIMIT = 1048576             # rocprim's radix_sort_config<>::merge_sort_limit: above it the sort is the onesweep radix sort


def _v(v):
    return np.ascontiguousarray(v, np.float32).reshape(-1, 3)


def _f(f):
    return np.ascontiguousarray(f, np.int32).reshape(-1, 3)


def tile(v, f, K, pad=0, interleave=False):
    """(vertices float32 [K nv + pad, 3], faces int32 [K nf, 3]) of K coincident copies; see the module's docstring"""
    v, f = _v(v), _f(f)
    nv, nf = len(v), len(f)
    assert K >= 1 and (K * nv + pad) < 2 ** 31 and nv > 0
    V = np.concatenate([np.tile(v, (K, 1)), np.repeat(v[:1], pad, 0)])
    F = f[None].astype(np.int64) + (np.arange(K, dtype=np.int64) * nv)[:, None, None]
    if interleave:
        F = F.transpose(1, 0, 2)
    return _v(V), _f(F.reshape(-1, 3))


def with_outliers(v, f, K, pad):
    """(vertices, faces, the two outliers): tile(v, f, K, pad) and two more unreferenced vertices, outside the box of the base on either
    side.  Coincident copies cannot notice a box that leaves vertices out -- every coordinate occurs K times; here the box is that of the
    last two vertices alone.  A law takes them as a pad of pad + 2 whose last two rows are the outliers, and the base is run with the
    absolute parameter that follows from the larger box."""
    V, F = tile(v, f, K, pad)
    lo, hi = _v(v).min(0).astype(np.float64), _v(v).max(0).astype(np.float64)
    out = np.float32([lo - [1.0, 2.0, 3.0], hi + [3.0, 1.0, 2.0]])
    return np.ascontiguousarray(np.concatenate([V, out])), F, out


def tile_rows(x, K, pad_row=None, pad=0):
    """a per-vertex (or per-edge, per-face) array repeated copy after copy, then `pad` rows of pad_row"""
    x = np.asarray(x)
    out = np.tile(x, (K,) + (1,) * (x.ndim - 1))
    if pad:
        out = np.concatenate([out, np.repeat(np.asarray(pad_row, x.dtype).reshape((1,) + x.shape[1:]), pad, 0)])
    return np.ascontiguousarray(out)


def face_position(nf, K, interleave=False):
    """[K, nf]: where face i of copy c lies in the tiled face array"""
    c, i = np.arange(K, dtype=np.int64)[:, None], np.arange(nf, dtype=np.int64)[None, :]
    return i * K + c if interleave else c * nf + i


def shift_keys(keys, nv, K):
    """the unique edge keys (a << 32) | b of the tiled mesh, ascending: the base's with a and b shifted by c nv, copy after copy"""
    k = np.asarray(keys, np.uint64).astype(np.int64)
    step = (np.arange(K, dtype=np.int64) * nv)[:, None]
    return np.ascontiguousarray((k[None, :] + (step << 32) + step).reshape(-1)).astype(np.uint64)


def two_block_vertices(v, n0, K, pad=0, pad_row=None):
    """a vertex array whose first n0 rows are per-copy block A and whose rest are per-copy block B -> all the copies' A (then the pad), then
    all the copies' B"""
    v = np.asarray(v)
    return np.ascontiguousarray(np.concatenate([tile_rows(v[:n0], K, pad_row, pad), tile_rows(v[n0:], K)]))


def two_block_faces(f, n0, n1, K, pad=0):
    """[K, nf, 3] int64: the base's faces over such a vertex array (n0 rows of block A, n1 of block B) as copy c holds them"""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    c = np.arange(K, dtype=np.int64)[:, None, None]
    return np.where(f[None] < n0, f[None] + c * n0, K * n0 + pad + c * n1 + (f[None] - n0))


def scaled(st, K, same=(), add=None):
    """a stats dict on the tiled mesh: every count K-fold, the keys of `same` as they are, `add` added afterwards"""
    out = {k: (x if k in same else K * x) for k, x in st.items()}
    for k, x in (add or {}).items():
        out[k] += x
    return out


def boundary_counts(nv, nf):
    """{name: K}: the largest K below and the smallest above each boundary, for a base of nv vertices and nf faces.  faces / vertices: the
    total 262144 (above: strictly more, so the boundary falls inside the last copy or in front of it); entries: 3 nf = 1048576 and below
    stays with the merge sort, above goes to the onesweep sort"""
    return dict(faces_below=(BOUNDARY - 1) // nf, faces_above=BOUNDARY // nf + 1, vertices_below=(BOUNDARY - 1) // nv, vertices_above=BOUNDARY // nv + 1,
                entries_below=MERGE_SORT_LIMIT // (3 * nf), entries_above=MERGE_SORT_LIMIT // (3 * nf) + 1)


# ---- clean -------------------------------------------------------------------------------------------------------------------------------------
def expected_components(want, nf, K, interleave=False):
    """mr.components.  Law: a component lies in one copy and its label is its lowest face, so label L of copy c becomes the position of
    face L of copy c (c nf + L; interleaved L K + c); -1 stays; the count is K-fold.  Reads no global."""
    lab, n = want
    pos = face_position(nf, K, interleave)
    out = np.full(K * nf, -1, np.int32)
    ok = lab >= 0
    out[pos[:, ok].ravel()] = pos[:, lab[ok]].ravel()
    return out, K * n


def expected_smooth(want, K, border):
    """mr.smooth and the border count.  Law: a vertex reads its own corner list and the edges' incidences, all of its copy: the positions
    repeat, the border vertices are K-fold.  Reads no global."""
    return tile_rows(want, K), K * border


def expected_clean(want, K):
    """mr.clean -> (vertices, faces, stats).  Law: every removal rule is local (components, duplicates, areas, edge incidences), the kept
    faces and used vertices are compacted in order, so copy c's output is the base's at c n_vertices / c n_faces.  Global read: the box of
    the smoothed vertices behind min_piece with relative = True -- coincident copies leave it, so `diameter` and `threshold` are the
    base's and every parameter is passed as it is."""
    ov, of, st = want
    faces = of[None].astype(np.int64) + (np.arange(K, dtype=np.int64) * len(ov))[:, None, None]
    return tile_rows(ov, K), _f(faces.reshape(-1, 3)), scaled(st, K, same=("diameter", "threshold"))


# ---- trim --------------------------------------------------------------------------------------------------------------------------------------
def expected_value_smooth(want, K):
    """mt.value_smooth.  Law: a vertex's sum runs over its own corner list: the values repeat.  Reads no global."""
    return tile_rows(want, K)


def split_ratio(want, ratio, K):
    """the island_ratio to pass for the tiled mesh.  Global read: a component moves when float(Q) < island_ratio float(Q_total), and the
    total area Q_total is K-fold on the tiled mesh; passing island_ratio / K restores the base's decisions.  (ratio / K) (K Q_total) need
    not round like ratio Q_total, so the decisions are compared here for every component of the base."""
    if ratio == 0.0:
        return 0.0
    qt = sum(want["Q"].values())
    for q in want["Q"].values():
        assert (float(q) < ratio * float(qt)) == (float(q) < (ratio / K) * float(K * qt)), (q, qt, ratio, K)
    return ratio / K


def expected_split(want, nv, nf, K):
    """mt.split -> dict(vertices, faces, src, side, label, stats, D2).  Law: the split mesh's vertices are the originals and then the cut
    vertices in key order, so copy-major within each block; the output keeps the used ones in order: all copies' kept originals, then all
    copies' kept cut vertices.  Faces copy-major, src shifted by c nf, label (the lowest split triangle of the component) by c times the
    base's split triangles.  Globals read: the box (D2: unchanged), min / max of the values (unchanged), and Q_total -- see split_ratio."""
    used = np.zeros(len(want["split_vertices"]), bool)
    used[want["split_faces"][want["split_final"] == 1].ravel()] = True
    n_out = len(want["vertices"])
    n0 = int(used[:nv].sum())
    assert n_out == int(used.sum())
    nT = len(want["split_faces"])
    c = np.arange(K, dtype=np.int64)[:, None]
    st = scaled(want["stats"], K)
    return dict(vertices=two_block_vertices(want["vertices"], n0, K), faces=_f(two_block_faces(want["faces"], n0, n_out - n0, K).reshape(-1, 3)),
                src=(want["src"][None] + c * nf).reshape(-1).astype(np.int32), side=tile_rows(want["side"], K),
                label=(want["label"][None] + c * nT).reshape(-1).astype(np.int32), stats=st, D2=want["D2"])


# ---- close -------------------------------------------------------------------------------------------------------------------------------------
def expected_border_loops(want, nf, K):
    """mc.border_loops -> (label, size, components).  Law: a border component lies in one copy, its label is its lowest entry 3 f + j:
    shifted by 3 c nf; sizes repeat; the count is K-fold.  Reads no global."""
    lab = want["label"].astype(np.int64)
    c = np.arange(K, dtype=np.int64)[:, None]
    return np.where(lab[None] >= 0, lab[None] + 3 * c * nf, -1).reshape(-1).astype(np.int32), tile_rows(want["size"], K), K * len(want["components"])


def expected_close_holes(want, nv, nf, K):
    """mc.close_holes -> (faces, stats); the vertices are the input's.  Law: the input's faces, then the new faces hole by hole in
    ascending label, and the labels ascend copy-major: copy c's new faces, shifted by c nv, follow copy c - 1's.  The forbidden diagonals
    are looked up in the edge table by keys of the hole's own copy.  Reads no global; the two `longest` figures are maxima and stay."""
    wv, wf, wst, info = want
    c = np.arange(K, dtype=np.int64)[:, None, None]
    old, new = wf[None, :nf].astype(np.int64) + c * nv, wf[None, nf:].astype(np.int64) + c * nv
    return _f(np.concatenate([old.reshape(-1, 3), new.reshape(-1, 3)])), scaled(wst, K, same=("longest_closed", "longest_loop"))


# ---- decimate ----------------------------------------------------------------------------------------------------------------------------------
def expected_quadrics(want, K, pad=0):
    """md.quadrics.  Law: the sum over a vertex's own corner list and its border edges: the rows repeat; an unreferenced (pad) vertex has
    the zero quadric.  Reads no global."""
    return tile_rows(want, K, np.zeros(10), pad)


def expected_costs(want, nv, K):
    """md.collapse_costs -> (key, multiplicity, cost, reject, position).  Law: every rule (locks, link condition, duplicates, placement,
    quality) reads the two stars of the edge, which lie in its copy; the unique edges in key order are the base's copy after copy with
    shifted keys.  Reads no global: the costs are not ranked here.  (The ranking is: see the module's docstring.)"""
    key, mult, cost, reject, pos = want[:5]
    return shift_keys(key, nv, K), tile_rows(mult, K), tile_rows(cost, K), tile_rows(reject, K), tile_rows(pos, K)


# ---- subdivide ---------------------------------------------------------------------------------------------------------------------------------
def expected_subdivide_stage(want, v, K, pad=0):
    """ms.loop_step's decisions -> dict(keys, multiplicity, split, odd, vertex_class, even).  Law: per unique edge in key order = copy after
    copy; per vertex repeated.  A pad vertex is in no face: locked, and stays where it is.  Global read: the box behind
    threshold_fraction -- unchanged, and the pad vertices lie on vertex 0."""
    v = _v(v)
    return dict(keys=shift_keys(want["keys"], len(v), K), multiplicity=tile_rows(want["multiplicity"], K), split=tile_rows(want["split"], K),
                odd=tile_rows(want["odd"], K), vertex_class=tile_rows(want["vertex_class"], K, 2, pad), even=tile_rows(want["even"], K, v[0], pad))


def children(want, f):
    """how many faces each face of the base becomes: 1 + its split edges (a face with a repeated index: 1)"""
    f = np.asarray(f, np.int64).reshape(-1, 3)
    ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    a, b = f, f[:, [1, 2, 0]]
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    is_split = np.isin(key, want["keys"][want["split"] != 0].astype(np.int64)) & ok[:, None]
    return 1 + is_split.sum(1)


def expected_subdivide(want, stats, v, f, K, pad=0, interleave=False):
    """one iteration of ms.subdivide, from loop_step's dict `want` and the whole call's stats -> (vertices, faces, stats).  Law: the even
    points of all copies first (then the pad), then the odd points copy by copy -- the r-th split edge in key order gets vertex nv + r, and
    the keys sort copy-major; the faces in input order, each replaced by its children: copy-major, copy c's at c nf_out; interleaved, the
    children of face i of copy c behind those of face i of the copies before it.  Global read: the box behind threshold_fraction
    (unchanged).  Stats: counts K-fold (a pad vertex is locked), iterations, threshold and max_valence the base's."""
    v, f = _v(v), _f(f)
    nv, nf = len(v), len(f)
    if stats["iterations"] == 0:
        V, F = tile(v, f, K, pad, interleave)
        return V, F, scaled(stats, K, same=("iterations", "threshold", "max_valence"), add=dict(n_vertices_in=pad, n_vertices=pad, locked_vertices=pad))
    assert stats["iterations"] == 1
    ns = want["n_split"]
    V = two_block_vertices(want["V"], nv, K, pad, v[0])
    F = two_block_faces(want["F"], nv, ns, K, pad)                                 # [K, nf_out, 3]
    if interleave:
        cnt = children(want, f)
        start = np.cumsum(cnt) - cnt
        assert int(cnt.sum()) == len(want["F"])
        owner = np.repeat(np.arange(nf), cnt)                                      # the base face of every output face
        within = np.arange(len(owner)) - start[owner]
        pos = K * start[owner][None, :] + np.arange(K, dtype=np.int64)[:, None] * cnt[owner][None, :] + within[None, :]
        out = np.zeros((K * len(owner), 3), np.int64)
        out[pos.ravel()] = F.reshape(-1, 3)
        F = out
    st = scaled(stats, K, same=("iterations", "threshold", "max_valence"), add=dict(n_vertices_in=pad, n_vertices=pad, locked_vertices=pad))
    return V, _f(F.reshape(-1, 3)), st


# ---- stitch and fill: the solve stages ---------------------------------------------------------------------------------------------------------
def expected_solve(want_x, K):
    """ms.solve's and mf.solve's x.  Law: a vertex's sums run over its own incidences; the per-vertex inputs (best view, colours, G; x and
    level) are tiled like the vertices, so x repeats.  Globals read: the largest degree (stitch) and L (fill) behind the Chebyshev
    coefficients -- maxima, unchanged.  The stitch's relative residual is a ratio of two norms that both grow by sqrt(K): the base's up to
    rounding, held as tests/test_gpu_meshstitch.py holds it."""
    return tile_rows(want_x, K)


# ---- the bases and the per-vertex inputs both test files use -----------------------------------------------------------------------------------
def _bases():
    import mesh_topology_fixtures as tf
    import meshclose_restatement as mc
    import meshdecimate_restatement as md
    import meshsubdivide_restatement as ms

    def messy():
        from test_gpu_meshdecimate import messy_mesh
        return messy_mesh()

    def layered():                                                                  # the height field with every face three times: nf / nv = 5.4, every
        v, f = md.grid_mesh(21, md.bumpy)                                           # edge in 3 or 6 faces, runs whose entries lie nf faces apart;
        return v, np.concatenate([f, [[0, 0, 1]], f, [[5, 5, 5]], f])               # and two faces with the sentinel keys
    return {"height_field": lambda: md.grid_mesh(21, md.bumpy), "cut_plane": mc.cut_plane, "annulus_16": lambda: mc.annulus(16),
            "book_in_grid_65": lambda: tf.get("book_in_grid_65"), "messy": messy, "patterns": ms.pattern_mesh, "layered": layered,
            "pieces": lambda: tf.get("pieces")}


_built = {}


def base(name):
    """(vertices, faces) of a base, built once, read-only"""
    if name not in _built:
        v, f = _bases()[name]()
        v, f = _v(v).copy(), _f(f).copy()
        v.setflags(write=False)
        f.setflags(write=False)
        _built[name] = (v, f)
    return _built[name]


ADAPTIVE_FRACTION = {"cut_plane": 0.11}    # the subdivision's threshold_fraction at which a base splits some edges and leaves others (default 0.04)
GROWING_THR = 3.0


def growing_hub(n=2060, seed=11):
    """a closed hub whose largest valence passes 4096 in the middle of a two-iteration call at the threshold GROWING_THR.  Vertex 0 over a
    rim of n vertices at radius 1 that zig-zags between z = 2 and z = -2, and an apex far below (z = -30).  Iteration 1: the spokes of
    vertex 0 (2.2 long) stay, the rim edges (4 long) split, so each of its faces becomes two that hold it: valence n -> 2 n; it does not
    move.  The rim vertices are interior and are drawn towards the apex, so in iteration 2 their spokes are longer than the threshold:
    vertex 0, now in 2 n > 4096 faces, is at an edge that splits and moves by beta_2n."""
    assert n % 2 == 0
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    t = 2.0 * np.pi * (i + rng.uniform(-0.2, 0.2, n)) / n
    rim = np.stack([np.cos(t), np.sin(t), np.where(i % 2 == 0, 2.0, -2.0) + rng.uniform(-0.05, 0.05, n)], 1)
    v = np.concatenate([[[0.01, -0.02, 0.0]], rim, [[0.0, 0.0, -30.0]]])
    f = np.concatenate([np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1), np.stack([np.full(n, n + 1), 1 + (i + 1) % n, 1 + i], 1)])
    return _v(v), _f(f)


def trim_values(nv, seed=8):
    """values round the trim value 7, even vertices above and odd ones below it: the cut passes through every star"""
    return 7.0 + np.where(np.arange(nv) % 2 == 0, 1.0, -1.0) * np.random.default_rng(seed).uniform(0.5, 1.5, nv)


def smooth_values(nv, seed=5):
    return np.random.default_rng(seed).normal(7.0, 2.0, size=nv)


def colouring(nv, seed=9):
    """(best view int32 [nv] in -1 .. 1 with vertices 0 and 1 coloured, colours uint8 [nv, 3], G float64 [nv, 3])"""
    rng = np.random.default_rng(seed)
    best = rng.integers(-1, 2, nv).astype(np.int32)
    best[:2] = (0, 1)
    return best, rng.integers(0, 256, (nv, 3)).astype(np.uint8), rng.normal(0.0, 20.0, (nv, 3))
