"""Scenes shared by tests/test_meshstitch_cpu.py and tests/test_gpu_meshstitch.py: caller-made colourings (best_view, rgb, G) on small
meshes -- no cameras -- and the independent evaluation of the Chebyshev polynomial."""
import numpy as np

import meshcolor_restatement as mr
import meshstitch_restatement as ms


def split_plane(nx=41, ny=31, offset=40, seed=5):
    """the nx x ny grid plane, the left columns coloured by view 0 and the right ones by view 1 = view 0 + offset over a random texture:
    (v, f, tex float64 [nv, 3], best int32, c uint8 [nv, 3])"""
    v, f = mr.grid_plane(nx, ny, 0.0, 0.0, 1.0, 10.0)
    tex = np.random.default_rng(seed).integers(0, 256 - offset, (len(v), 3)).astype(np.float64)
    right = (np.arange(len(v)) % nx) >= nx // 2
    return v, f, tex, right.astype(np.int32), (tex + offset * right[:, None]).astype(np.uint8)


def true_texture_G(f, best, tex):
    """G where every target difference, across the seam too, is the true texture's: (G, Incidences)"""
    inc = ms.Incidences(f, np.asarray(best) >= 0)
    return inc.ordered_sum(tex[inc.I] - tex[inc.J]), inc


def planted_plane(nx=41, ny=31, seed=7):
    """the split plane with everything a gather can trip over planted in it: its border; an edge with three faces (a fin on an interior
    edge, whose apex is an extra vertex); a face with a repeated index; an unreferenced vertex; a column of uncoloured vertices that
    splits the plane in two components (the seam lies inside the right one); and a coloured vertex whose neighbours are all uncoloured
    (deg = 0).  G is random half-integers, 0 where deg = 0: the solve stage takes it as given.  (f, best, c, G, marks dict)"""
    v, f, tex, best, c = split_plane(nx, ny, 40, seed)
    nv0 = len(v)
    rng = np.random.default_rng(seed + 1)
    apex, loose = nv0, nv0 + 1
    e0, e1 = 5 * nx + 7, 5 * nx + 8                          # an interior edge: two faces of the plane, and the fin
    extra = np.int32([[e0, e1, apex], [3, 3, 4], [9, 10, 9]])
    f = np.concatenate([f, extra]).astype(np.int32)
    best = np.concatenate([best, [0, 1]]).astype(np.int32)   # the apex and the unreferenced vertex are coloured
    c = np.concatenate([c, [[200, 10, 90], [1, 2, 3]]]).astype(np.uint8)
    wall = 12                                                # the uncoloured column
    best[np.arange(ny) * nx + wall] = -1
    lone = 20 * nx + 30                                      # a coloured vertex in a ring of uncoloured ones
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                best[lone + dy * nx + dx] = -1
    G = rng.integers(-200, 201, (len(best), 3)).astype(np.float64) / 2.0
    G[[lone, loose]] = 0.0                                   # (a vertex without incidences has no target difference)
    return f, best, c, G, dict(apex=apex, loose=loose, lone=lone, wall=wall, fin_edge=(e0, e1), nx=nx, ny=ny)


def acosh1p(e):
    """acosh(1 + e) without the cancellation of 1 + e - 1"""
    return np.log1p(e + np.sqrt(e * (e + 2.0)))


def cheb_closed(sigma, k):
    """T_k(sigma) = cosh(k acosh sigma), sigma in [1, 2): sigma - 1 is exact there"""
    return float(np.cosh(k * acosh1p(sigma - 1.0)))
