"""Meshes whose topology is unfriendly on purpose, for the mesh units' shared topology layer (csrc/mesh_common.h, csrc/dev_prims.h): one
vertex in hundreds of faces, one edge in hundreds of faces, strips whose neighbouring faces lie thousands of indices apart, pieces whose
ends fall on 255 / 256 / 257 in face index, and vertex counts of 2^k - 1, 2^k, 2^k + 1 together with faces that repeat an index.

Test infrastructure only, plain numpy: tests/test_mesh_topology_cpu.py asserts what each builder reaches and holds the restatements to
independent definitions on them; tests/test_gpu_mesh_topology.py runs the stages on them.  Every builder returns (float32 vertices [nv, 3],
int32 faces [nf, 3]), is seeded, and is non-planar, so that cotangents, quadrics and areas are not trivially equal."""
from __future__ import annotations

import numpy as np

HUB_SIZES = (63, 64, 65, 255, 256, 257)
BOOK_SIZES = (3, 64, 65, 256, 257, 300, 1000)
PADDED_SIZES = (255, 256, 257, 65535, 65536, 65537)
STRIP_ORDERS = ("ascending", "descending", "even_odd", "shuffled")
PIECE_SIZES = (255, 1, 256, 2, 257, 64, 65, 63, 300)
GRID_N = 12
SPINE_IN_GRID = (0, 1)                                    # book_in_grid's spine: the grid's interior edge between lattice points (5, 5) and (6, 5)
_SPINE_LATTICE = (5 * GRID_N + 5, 5 * GRID_N + 6)


def _f32(v):
    return np.ascontiguousarray(v, np.float32).reshape(-1, 3)


def _i32(f):
    return np.ascontiguousarray(f, np.int32).reshape(-1, 3)


def hub(n, closed=False, seed=1):
    """vertex 0 over a rim 1 .. n: the n faces (0, 1 + i, 1 + (i + 1) % n).  closed: vertex n + 1 below the rim and the n faces
    (n + 1, 1 + (i + 1) % n, 1 + i) after them -- a closed manifold of 2 n faces.  Open, the border is one loop of n entries."""
    rng = np.random.default_rng(seed + 7 * n)
    t = 2.0 * np.pi * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
    r = rng.uniform(0.8, 1.2, n)
    rim = np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-0.15, 0.15, n)], 1)
    i = np.arange(n)
    v = [[[0.03, -0.02, 0.9]], rim]
    f = [np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1)]
    if closed:
        v.append([[-0.04, 0.05, -1.1]])
        f.append(np.stack([np.full(n, n + 1), 1 + (i + 1) % n, 1 + i], 1))
    return _f32(np.concatenate(v)), _i32(np.concatenate(f))


def book(n, duplicates=0, sides=None, seed=2):
    """n pages on the spine edge (0, 1): page i is (0, 1, 2 + i) where sides[i] == 0 and (1, 0, 2 + i) where it is 1; sides defaults to
    i & 1 (odd pages wound the other way).  duplicates = d repeats the first d pages as the last d faces, on the same three vertices:
    duplicate k rotated (k even) or with its winding reversed (k odd) -- in the spine's run it lies n entries behind its original."""
    rng = np.random.default_rng(seed + 7 * n)
    sides = (np.arange(n) & 1) if sides is None else np.asarray(sides, np.int64).reshape(n)
    t = 2.0 * np.pi * (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
    r = rng.uniform(0.8, 1.2, n)
    pages = np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(0.2, 0.8, n)], 1)
    v = np.concatenate([[[0.01, 0.02, 0.0], [-0.02, 0.01, 1.0]], pages])
    p = 2 + np.arange(n)
    f = np.where(sides[:, None] == 0, np.stack([np.zeros(n, np.int64), np.ones(n, np.int64), p], 1), np.stack([np.ones(n, np.int64), np.zeros(n, np.int64), p], 1))
    dup = [f[k][[1, 2, 0]] if k % 2 == 0 else f[k][[0, 2, 1]] for k in range(duplicates)]
    return _f32(v), _i32(np.concatenate([f, np.array(dup, np.int64).reshape(-1, 3)]))


def grid(nx=GRID_N, ny=GRID_N, seed=3):
    """a jittered nx x ny lattice, every square cut along the same diagonal: (i, i + 1, i + nx + 1), then (i, i + nx + 1, i + nx)"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    v = np.stack([x.ravel() + rng.uniform(-0.2, 0.2, nx * ny), y.ravel() + rng.uniform(-0.2, 0.2, nx * ny), rng.uniform(-0.3, 0.3, nx * ny)], 1)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)).ravel()
    return _f32(v), _i32(np.concatenate([np.stack([i, i + 1, i + nx + 1], 1), np.stack([i, i + nx + 1, i + nx], 1)]))


def book_in_grid(n, seed=4):
    """the 12 x 12 grid with n pages on its interior edge SPINE_IN_GRID = (a, b), incidence n + 2: page k is (a, b, 144 + k) for even k,
    (b, a, 144 + k) for odd k, and sits at face index (k * nf) // n of the nf = 242 + n faces -- interleaved with the grid's faces.  The
    grid's vertices are numbered row by row, except that the spine's two lattice points change numbers with the first two: the spine is
    (0, 1), so that the two lowest vertices are interior ones whose corner lists run through the whole face array (what sorts next to
    vertex 0 by mistake -- a sentinel key cut to too few bits -- lands in lists that every stage reads)."""
    rng = np.random.default_rng(seed + 7 * n)
    gv, gf = grid()
    swap = np.arange(len(gv))
    swap[list(_SPINE_LATTICE)], swap[[0, 1]] = (0, 1), _SPINE_LATTICE
    gv, gf = gv[swap], swap[gf]                                                 # (swap is its own inverse)
    a, b = SPINE_IN_GRID
    mid = 0.5 * (gv[a].astype(np.float64) + gv[b].astype(np.float64))
    t = np.pi * (np.arange(n) + 0.5 + rng.uniform(-0.3, 0.3, n)) / n
    r = rng.uniform(0.8, 1.2, n)
    pv = mid + np.stack([rng.uniform(-0.2, 0.2, n), r * np.cos(t), 0.5 + r * np.sin(t)], 1)       # above the grid, fanned round the edge
    k = np.arange(n)
    pf = np.where((k & 1)[:, None] == 0, np.stack([np.full(n, a), np.full(n, b), 144 + k], 1), np.stack([np.full(n, b), np.full(n, a), 144 + k], 1))
    nf = len(gf) + n
    f = np.zeros((nf, 3), np.int64)
    at = (k * nf) // n
    is_page = np.zeros(nf, bool)
    is_page[at] = True
    f[is_page], f[~is_page] = pf, gf
    return _f32(np.concatenate([gv, pv])), _i32(f)


def book_in_grid_pages(n):
    """the face indices of book_in_grid(n)'s pages"""
    return (np.arange(n) * (2 * (GRID_N - 1) ** 2 + n)) // n


def _strip_faces(n, first=0):
    k = np.arange(n)
    return first + np.where((k & 1)[:, None] == 0, np.stack([k, k + 1, k + 2], 1), np.stack([k + 1, k, k + 2], 1))


def _strip_points(n, rng):
    k = np.arange(n + 2)
    return np.stack([0.5 * k + rng.uniform(-0.1, 0.1, n + 2), (k & 1) + rng.uniform(-0.1, 0.1, n + 2), rng.uniform(-0.2, 0.2, n + 2)], 1)


def strip_order(n, order, seed=5):
    """position -> strip face of the face array in the given order"""
    if order == "ascending":
        return np.arange(n)
    if order == "descending":
        return np.arange(n)[::-1].copy()
    if order == "even_odd":
        return np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    assert order == "shuffled"
    return np.random.default_rng(seed).permutation(n)


def strip(n=4096, order="ascending", seed=5):
    """a consistently wound triangle strip of n faces over n + 2 jittered points, strip face k = (k, k + 1, k + 2) (odd k: (k + 1, k, k + 2)),
    its face array in one of STRIP_ORDERS.  One piece; its border is one loop of n + 2 entries."""
    v = _strip_points(n, np.random.default_rng(seed))
    return _f32(v), _i32(_strip_faces(n)[strip_order(n, order, seed)])


def pieces(sizes=PIECE_SIZES, seed=6):
    """disjoint strips of the given face counts laid end to end in the face array, piece p moved to x = 1000 p; a strip of m faces is about
    m / 2 long, so the diameters grow with the size"""
    rng = np.random.default_rng(seed)
    v, f, nv = [], [], 0
    for p, m in enumerate(sizes):
        v.append(_strip_points(m, rng) + np.array([1000.0 * p, 0.0, 0.0]))
        f.append(_strip_faces(m, nv))
        nv += m + 2
    return _f32(np.concatenate(v)), _i32(np.concatenate(f))


def piece_bounds(sizes=PIECE_SIZES):
    """the first face of every piece, and the end of the last"""
    return np.concatenate([[0], np.cumsum(sizes)])


def piece_diameters(v, f, sizes=PIECE_SIZES):
    """the fp64 diagonal of every piece's float32 box"""
    b = piece_bounds(sizes)
    out = []
    for p in range(len(sizes)):
        q = v[np.unique(f[b[p]:b[p + 1]])].astype(np.float64)
        d = q.max(0) - q.min(0)
        out.append(float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
    return np.array(out)


def padded(v, f, nv):
    """the same mesh with nv vertices: unreferenced, finite, distinct vertices appended; corner 1 of face 2 nf // 3 re-pointed to vertex
    nv - 1, which gets the position of the vertex it replaces; and the repeated-index faces [a, a, b] (a, b = face 0's first two) and
    [c, c, c] (c = nv - 1) inserted at nf // 2.  Returns (vertices, faces)."""
    v, f = _f32(v), _i32(f)
    n0, nf = len(v), len(f)
    assert nv > n0
    k = np.arange(nv - n0)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    pad = np.stack([lo[0] + (k % 256) * (hi[0] - lo[0]) / 256.0, lo[1] + (k // 256) * (hi[1] - lo[1]) / 256.0, np.full(len(k), hi[2] + 0.25)], 1)
    V = np.concatenate([v, pad.astype(np.float32)])
    F = f.copy()
    V[nv - 1] = V[F[2 * nf // 3, 1]]
    F[2 * nf // 3, 1] = nv - 1
    a, b = int(f[0, 0]), int(f[0, 1])
    F = np.concatenate([F[:nf // 2], [[a, a, b], [nv - 1, nv - 1, nv - 1]], F[nf // 2:]])
    return _f32(V), _i32(F)


def pillow(nv):
    """the two faces (0, 2, 1), (0, 3, 2) under a square hole 0 - 1 - 2 - 3 whose corners 1 and 3 stand high, then the repeated-index face
    [1, 1, 2], over nv vertices (4 .. nv - 1 unreferenced): the fill's cheaper diagonal (0, 2) is an edge of the mesh, which the fill has to
    find in the sorted edge table -- behind whatever sorts in front of vertex 0's keys"""
    assert nv > 4
    k = np.arange(nv - 4)
    pad = np.stack([2.0 + (k % 256) / 256.0, (k // 256) / 256.0, np.full(len(k), -0.5)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.0], [1.05, 0.02, 1.0], [1.0, 1.0, 0.1], [-0.03, 0.95, 1.1]], pad])
    return _f32(v), _i32([[0, 2, 1], [0, 3, 2], [1, 1, 2]])


class SortedPositions:
    """Where the runs and the lists lie in the stably sorted tables, by the key definitions of k_mesh_edge_keys / k_mesh_corner_keys: entry
    3 f + j has the edge key (min << 32) | max of (v_j, v_j+1) and the corner key v_j; every entry of a face with a repeated index has the
    keys nv << 32 and nv, which sort behind all others.
      edge_key, edge_val        the sorted edge table
      run_key, run_start, run_end   every run of equal edge keys, [start, end)
      corner_val                the sorted corner table
      list_start [nv + 2]       vertex v's corner list is [list_start[v], list_start[v + 1]); v = nv: the entries of the repeated-index faces"""

    def __init__(self, f, nv):
        f = np.asarray(f, np.int64).reshape(-1, 3)
        ok = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
        a, b = f, f[:, [1, 2, 0]]
        ekey = np.where(ok[:, None], (np.minimum(a, b) << 32) | np.maximum(a, b), np.int64(nv) << 32).ravel()
        o = np.argsort(ekey, kind="stable")
        self.edge_key, self.edge_val = ekey[o], o
        first = np.ones(len(o), bool)
        first[1:] = self.edge_key[1:] != self.edge_key[:-1]
        self.run_start = np.nonzero(first)[0]
        self.run_end = np.concatenate([self.run_start[1:], [len(o)]]).astype(np.int64)
        self.run_key = self.edge_key[self.run_start]
        ckey = np.where(ok[:, None], f, nv).ravel()
        o = np.argsort(ckey, kind="stable")
        self.corner_val = o
        self.list_start = np.searchsorted(ckey[o], np.arange(nv + 2))

    def run(self, a, b):
        """[start, end) of the run of edge (a, b)"""
        i = int(np.searchsorted(self.run_key, (min(a, b) << 32) | max(a, b)))
        assert self.run_key[i] == (min(a, b) << 32) | max(a, b)
        return int(self.run_start[i]), int(self.run_end[i])

    def list(self, v):
        return int(self.list_start[v]), int(self.list_start[v + 1])

    def longest_run(self):
        return int((self.run_end - self.run_start).max())


def sorted_positions(f, nv):
    return SortedPositions(f, nv)


def straddles(start, end, m):
    """[start, end) holds a position p > start that is a multiple of m: the range lies in more than one block of m"""
    return (end - 1) // m > start // m


# ---- the catalogue: name -> (vertices, faces), built once ----------------------------------------------------------------------------------
def _catalogue():
    c = {}
    for n in HUB_SIZES:
        c["hub_%d" % n] = lambda n=n: hub(n)
        c["hub_%d_closed" % n] = lambda n=n: hub(n, closed=True)
    c["hub_1000"] = lambda: hub(1000)
    for n in BOOK_SIZES:
        c["book_%d" % n] = lambda n=n: book(n)
        c["book_%d_dup" % n] = lambda n=n: book(n, duplicates=2)
    for n in (65, 257):
        c["book_in_grid_%d" % n] = lambda n=n: book_in_grid(n)
    for o in STRIP_ORDERS:
        c["strip_%s" % o] = lambda o=o: strip(4096, o)
    c["pieces"] = pieces
    for nv in PADDED_SIZES:
        c["padded_%d_book_in_grid_65" % nv] = lambda nv=nv: padded(*book_in_grid(65), nv)
    for nv in (256, 65536):
        c["padded_%d_hub_65_closed" % nv] = lambda nv=nv: padded(*hub(65, closed=True), nv)
    for nv in (255, 256, 257, 65536):
        c["pillow_%d" % nv] = lambda nv=nv: pillow(nv)
    return c


CATALOGUE = _catalogue()
_built = {}


def get(name):
    """(vertices, faces) of a catalogue entry; built once, handed out read-only"""
    if name not in _built:
        v, f = CATALOGUE[name]()
        v.setflags(write=False)
        f.setflags(write=False)
        _built[name] = (v, f)
    return _built[name]


def names(*prefixes):
    return [n for n in CATALOGUE if n.startswith(prefixes)]
