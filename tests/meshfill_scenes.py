"""Fixtures shared by tests/test_meshfill_cpu.py and tests/test_gpu_meshfill.py: caller-made colourings (faces, rgb, best_view) on small
meshes -- no cameras.  Every fixture is (f int32 [nf, 3], rgb uint8 [nv, 3], best int32 [nv]); an unknown vertex carries (127, 127, 127)."""
import numpy as np

import meshcolor_restatement as mr
import meshstitch_scenes as sc

NX, NY = 41, 31


def _grey(rgb, best):
    rgb = np.array(rgb, np.uint8)
    rgb[np.asarray(best) < 0] = mr.GREY
    return rgb


def plane(unknown, seed=11):
    """meshstitch_scenes' 41 x 31 plane under a random texture; unknown: bool [ny, nx]"""
    _, f = mr.grid_plane(NX, NY, 0.0, 0.0, 1.0, 10.0)
    rgb = np.random.default_rng(seed).integers(0, 256, (NX * NY, 3)).astype(np.uint8)
    best = np.where(np.asarray(unknown).ravel(), -1, 0).astype(np.int32)
    return f, _grey(rgb, best), best


def disc(radius):
    ys, xs = np.mgrid[0:NY, 0:NX]
    return (xs - NX // 2) ** 2 + (ys - NY // 2) ** 2 <= radius * radius


def plane_disc(radius=8):
    return plane(disc(radius))


def plane_left_columns(columns=3):
    return plane(np.mgrid[0:NY, 0:NX][1] >= columns)


def plane_ramp(radius=8):
    """the plane coloured 3 x + 2 y (at most 180), a disc of it unknown"""
    f, _, best = plane_disc(radius)
    ys, xs = np.mgrid[0:NY, 0:NX]
    ramp = (3 * xs + 2 * ys).ravel()
    return f, _grey(np.stack([ramp, ramp + 1, 255 - ramp], axis=1), best), best


def strip(n, both_ends=True, seed=3):
    """a triangle strip of n vertices, faces (i, i + 1, i + 2); known: its first two vertices and, with both_ends, its last two"""
    i = np.arange(n - 2)
    f = np.stack([i, i + 1, i + 2], axis=1).astype(np.int32)
    best = np.full(n, -1, np.int32)
    best[:2] = 0
    if both_ends:
        best[-2:] = 1
    return f, _grey(np.random.default_rng(seed + n).integers(0, 256, (n, 3)), best), best


def strip_of_rounds(L):
    """a strip known at one end whose front takes exactly L rounds"""
    return strip(2 + 2 * L, False)


def soup(nv=257, nf=700, known=0.3, seed=101):
    """random faces over nv vertices: random valences, faces with a repeated index, vertices no face holds"""
    rng = np.random.default_rng(seed + nv)
    f = rng.integers(0, nv, (nf, 3)).astype(np.int32)
    best = np.where(rng.random(nv) < known, rng.integers(0, 4, nv), -1).astype(np.int32)
    return f, _grey(rng.integers(0, 256, (nv, 3)), best), best


def hub(n=1000, seed=17):
    """a closed fan: the unknown vertex 0 in n faces (2 n incidences, summed in order), a rim of known vertices with a run of five unknown ones"""
    rim = 1 + np.arange(n)
    f = np.stack([np.zeros(n, np.int64), rim, 1 + (rim % n)], axis=1).astype(np.int32)
    best = np.zeros(n + 1, np.int32)
    best[0] = -1
    best[400:405] = -1
    return f, _grey(np.random.default_rng(seed).integers(0, 256, (n + 1, 3)), best), best


def planted():
    """meshstitch_scenes' planted plane (a three-face edge, faces with a repeated index, an unreferenced known vertex, an unknown column and
    an unknown ring) with an unreferenced unknown vertex and a triangle of three unknown vertices, a component without a known one, appended:
    (f, rgb, best, marks)"""
    f, best, c, _, marks = sc.planted_plane()
    n = len(best)
    f = np.concatenate([f, [[n + 1, n + 2, n + 3]]]).astype(np.int32)
    best = np.concatenate([best, [-1, -1, -1, -1]]).astype(np.int32)
    c = np.concatenate([c, np.full((4, 3), mr.GREY, np.uint8)])
    return f, _grey(c, best), best, dict(marks, loose_unknown=n, island=(n + 1, n + 2, n + 3))


# the fixtures the restatement is held to the direct solver on, with the call's max_rounds
EXACT_FIXTURES = {
    "disc8": (plane_disc, (8,), 0),
    "disc10_cap3": (plane_disc, (10,), 3),
    "left_columns": (plane_left_columns, (), 0),
    "strip40": (strip, (40,), 0),
    "strip200": (strip, (200,), 0),
    "strip600": (strip, (600,), 0),
    "strip200_one_end": (strip, (200, False), 0),
    "soup257": (soup, (), 0),
}


def fixture(name):
    fn, args, max_rounds = EXACT_FIXTURES[name]
    return fn(*args) + (max_rounds,)
