"""The numpy restatement of the mesh smoothing and clean-up (tests/meshclean_restatement.py) against known answers.
No GPU: what the GPU tests hold the kernels to is itself checked here against hand-computed points, a brute-force border rule, scipy's
connected components and the noisy sphere of the Poisson tests."""
import collections

import numpy as np
import pytest

import meshclean_restatement as mr
import poisson_restatement as pr


def edge_faces(faces):
    """undirected edge -> the faces on it, by brute force"""
    d = collections.defaultdict(list)
    for i, (a, b, c) in enumerate(np.asarray(faces).tolist()):
        if a != b and b != c and a != c:
            for u, v in ((a, b), (b, c), (c, a)):
                d[(min(u, v), max(u, v))].append(i)
    return d


@pytest.mark.parametrize("cotangent", [False, True])
def test_interior_vertices_of_a_flat_regular_grid_do_not_move(cotangent):
    """Right isosceles triangles: the cotangents are exactly 1 and 0 and every sum is one of small integers, so "do not move" is exact."""
    v, f = mr.grid_mesh(7, 6)
    _, border = mr.incidences(f, len(v))
    assert border.sum() == 2 * 7 + 2 * 6 - 4
    for steps in (1, 3):
        p = mr.smooth(v, f, steps, cotangent, boundary=False)
        assert np.array_equal(p, v)
    p = mr.smooth(v, f, 1, cotangent, boundary=True)
    assert np.array_equal(p[~border], v[~border])


def test_apex_of_a_regular_fan_lands_at_the_hand_computed_point():
    # umbrella: each of the n ring vertices is added once per face it shares with the apex, twice; the ring sums to 0:
    # P' = ((0, 0, 1) + 0) / (1 + 2 n) = (0, 0, 1 / 13) for n = 6
    v, f = mr.fan_mesh(6)
    p = mr.smooth(v, f, 1, cotangent=False)
    assert abs(p[0, 2] - 1.0 / 13.0) <= 1e-7 and np.abs(p[0, :2]).max() <= 1e-7
    # cotangent, n = 4, ring (+-1, 0, 0), (0, +-1, 0), apex (0, 0, 1): the corner opposite an apex edge lies between (0, -1, 1) and (1, -1, 0):
    # dot 1, |cross| = |(1, 1, 1)| = sqrt 3; each ring vertex gets two such weights, W = 8 / sqrt 3, S = 0: z' = 1 / (1 + 8 / sqrt 3)
    v, f = mr.fan_mesh(4)
    p = mr.smooth(v, f, 1, cotangent=True)
    assert abs(p[0, 2] - 1.0 / (1.0 + 8.0 / np.sqrt(3.0))) <= 1e-7 and np.abs(p[0, :2]).max() <= 1e-7
    # the ring vertices are border vertices: with boundary = 0 they stay
    assert np.array_equal(mr.smooth(v, f, 1, True, boundary=False)[1:], v[1:])


def test_border_vertices_of_an_open_strip_follow_the_1d_rule():
    n = 9
    x = np.arange(n, dtype=np.float64) ** 2                      # uneven spacing: the rule moves every vertex
    v = np.concatenate([np.stack([x, np.zeros(n), np.zeros(n)], 1), np.stack([x + 0.25, np.ones(n), 0.5 * np.ones(n)], 1)]).astype(np.float32)
    i = np.arange(n - 1)
    f = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i, i + n + 1, i + n], 1)]).astype(np.int32)
    _, border = mr.incidences(f, len(v))
    assert border.all()
    nb = collections.defaultdict(list)
    for (a, b), fs in edge_faces(f).items():
        if len(fs) == 1:
            nb[a].append(b)
            nb[b].append(a)
    p = mr.smooth(v, f, 1, cotangent=True, boundary=True)
    v64 = v.astype(np.float64)
    for q in range(len(v)):
        m = len(nb[q])
        assert m == 2
        want = (2.0 * v64[q] + v64[nb[q]].sum(0)) / (2.0 + m)
        assert np.abs(p[q] - want).max() <= 1e-6 * max(1.0, np.abs(want).max()), q
    assert p[3, 0] == np.float32(9.5)                             # (2 * 9 + 4 + 16) / 4
    assert np.array_equal(mr.smooth(v, f, 2, True, boundary=False), v)


def pieces_mesh():
    """four pieces: a grid, a second grid that touches the first at ONE shared vertex only, a fan far away, a face with a repeated index"""
    v1, f1 = mr.grid_mesh(4, 4)
    v2, f2 = mr.grid_mesh(3, 3)
    v2 = v2 + np.float32([3.0, 3.0, 0.0])                         # its vertex 0 = the first grid's last vertex (3, 3, 0)
    f2 = f2 + len(v1)
    f2[f2 == len(v1)] = len(v1) - 1                               # share that vertex
    v3, f3 = mr.fan_mesh(5)
    v3 = v3 + np.float32([20.0, 0.0, 0.0])
    f3 = f3 + len(v1) + len(v2)
    v = np.concatenate([v1, v2, v3])
    f = np.concatenate([f3[:2], f1, [[0, 0, 1]], f2, f3[2:]]).astype(np.int32)
    return v, f


def test_labels_agree_with_scipys_connected_components():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    for v, f in (pieces_mesh(), mr.grid_mesh(9, 5), mr.fan_mesh(7)):
        nf = len(f)
        pairs = [(a, b) for fs in edge_faces(f).values() for a in fs for b in fs if a < b]
        r, c = (np.array([p[k] for p in pairs], np.int64) for k in range(2))
        n, lab = connected_components(coo_matrix((np.ones(len(r)), (r, c)), shape=(nf, nf)), directed=False)
        lowest = np.full(n, nf)
        np.minimum.at(lowest, lab, np.arange(nf))
        want = lowest[lab]
        bad = ~mr.distinct(f)
        want[bad] = -1
        got, ncomp = mr.components(f)
        assert np.array_equal(got, want)
        assert ncomp == n - int(bad.sum())
    v, f = pieces_mesh()
    got, ncomp = mr.components(f)
    assert ncomp == 3 and len(set(got.tolist())) == 4             # the two grids stay apart although they share a vertex


@pytest.fixture(scope="module")
def sphere5():
    xyz, nrm = pr.sphere_samples(20000)
    return pr.reconstruct(xyz, nrm, 5)


def test_five_cotangent_steps_lower_the_spheres_radial_error(sphere5):
    R = sphere5
    p = mr.smooth(R["verts"], R["faces"], 5, cotangent=True, boundary=True)
    assert np.isfinite(p).all()
    before, after = pr.radial_error_h(R["verts"], R["h"]), pr.radial_error_h(p, R["h"])
    print("depth 5: max radial error %.4f h -> %.4f h, mean %.4f h -> %.4f h" % (before.max(), after.max(), before.mean(), after.mean()))
    assert after.max() < before.max()
    assert not mr.incidences(R["faces"], len(p))[1].any()         # closed: no border vertex


def test_the_clean_up_fixture_exercises_every_rule(sphere5):
    R = sphere5
    nv, nf = len(R["verts"]), len(R["faces"])
    V, F, expect = mr.cleanup_fixture(R["verts"], R["faces"])
    v, f, st = mr.clean(V, F, smooth_steps=0)
    got = {k: st[k] for k in expect}
    assert got == expect and all(n > 0 for n in got.values())
    assert expect["removed_isolated"] == nf == 23792
    assert st["components"] == 4 and st["components_removed"] == 1      # sphere (+ duplicates + fin), 5 % copy, 20 % copy, the collinear face
    assert len(f) == len(F) - sum(expect.values()) == 2 * nf - 2
    # the 5 % copy, the collinear face's three vertices and the fin's tip go; the repeated-index face used the sphere's vertices
    assert st["vertices_dropped"] == nv + 3 + 1 and len(v) == 2 * nv
    assert st["border_vertices"] == 3 + 3                               # the collinear face's vertices and the fin's (two of its edges have one face)
    # each switch, turned off, leaves its faces in
    assert mr.clean(V, F, 0, duplicates=False, nonmanifold=False)[2]["removed_duplicate"] == 0
    assert mr.clean(V, F, 0, zero_area=False)[2]["n_faces"] == len(f) + 2
    assert mr.clean(V, F, 0, nonmanifold=False)[2]["n_faces"] == len(f) + 3
    s0 = mr.clean(V, F, 0, min_piece=0.0)[2]
    # (the 5 % copy's smallest slivers collapse in float32: left in, some of its faces go as zero-area faces instead)
    assert s0["removed_isolated"] == 0 and s0["components_removed"] == 0 and s0["n_faces"] == len(f) + nf - (s0["removed_zero_area"] - 2)
    # with the duplicates left in, their edges carry three faces: rule 4 takes the pair and the three neighbours of each
    assert mr.clean(V, F, 0, duplicates=False)[2]["removed_nonmanifold"] > 3
