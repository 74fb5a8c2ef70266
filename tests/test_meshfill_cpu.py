"""The numpy restatement of the colour fill (tests/meshfill_restatement.py) against what does not depend on it: the
assembled system through scipy's direct solver, a breadth-first search in plain Python, and known answers.  No GPU."""
import numpy as np
import pytest

import meshfill_restatement as mf
import meshfill_scenes as fs
import meshstitch_scenes as sc

_cache = {}


def filled_fixture(name):
    """a fixture of fs.EXACT_FIXTURES through the whole restated call at the defaults, computed once: a dict the tests only read"""
    if name not in _cache:
        f, rgb, best, max_rounds = fs.fixture(name)
        out, level, st, x, x0 = mf.fill(f, rgb, best, max_rounds)
        _cache[name] = dict(f=f, rgb=rgb, best=best, max_rounds=max_rounds, out=out, level=level, st=st, x=x, x0=x0)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(fs.EXACT_FIXTURES))
def test_default_steps_come_within_half_a_level_of_the_direct_solve(name):
    r = filled_fixture(name)
    st = r["st"]
    want = mf.exact(r["f"], r["x0"], r["level"], st["rounds"])
    filled = (r["level"] >= 1)
    err = float(np.abs(r["x"] - want)[filled].max())
    print("%s: %d filled of %d unknown, L %d, %d steps, largest |x - x*| %.3g, largest |x_front - x*| %.3g"
          % (name, st["filled"], st["filled"] + st["unreached"], st["rounds"], st["steps"], err, float(np.abs(r["x0"] - want)[filled].max())))
    assert st["filled"] > 0 and st["steps"] == mf.auto_steps(st["rounds"], 1e-4)
    assert err <= 0.5
    assert (r["x"][~filled] == r["rgb"].astype(np.float64)[~filled]).all()
    # every filled byte within one level of the rounded exact solution, every other byte the input's
    assert np.abs(r["out"].astype(int) - np.floor(want + 0.5).astype(int))[filled].max() <= 1
    assert r["out"][~filled].tobytes() == r["rgb"][~filled].tobytes()
    if name == "disc10_cap3":
        assert st["rounds"] == 3 and st["unreached"] > 0 and (r["out"][r["level"] < 0] == 127).all()
        # the incidences to unreached neighbours are dropped: fewer kept than a filled vertex has
        assert st["incidences"] < mf.all_incidences(r["f"], len(r["best"])).deg[filled].sum()
    elif name != "soup257":
        assert st["unreached"] == 0


def test_the_step_count_is_the_least_that_reaches_the_reduction():
    r = filled_fixture("strip600")
    L = r["st"]["rounds"]
    assert L == 149 and r["st"]["steps"] == 2101              # about 14 (L + 1)
    sigma = mf.spectrum(mf.lmin_of(L))[2]
    k = r["st"]["steps"]
    assert sc.cheb_closed(sigma, k) >= 1e4 * (1 - 1e-9) and sc.cheb_closed(sigma, k - 1) < 1e4 * (1 + 1e-9)
    with pytest.raises(ValueError):
        mf.auto_steps(10 ** 6, 1e-4)


def test_levels_are_the_breadth_first_distance():
    for name in sorted(fs.EXACT_FIXTURES):
        r = filled_fixture(name)
        assert r["level"].tobytes() == mf.bfs_levels(r["f"], r["best"], r["max_rounds"]).tobytes(), name
    f, rgb, best = fs.hub()
    x, level, L = mf.front(f, rgb, best)
    assert level.tobytes() == mf.bfs_levels(f, best).tobytes() and L == 2 and level[0] == 1 and level[402] == 2
    for cap in (1, 2, 5):
        f, rgb, best = fs.plane_left_columns()
        assert mf.front(f, rgb, best, cap)[1].tobytes() == mf.bfs_levels(f, best, cap).tobytes()


def test_front_values_lie_in_the_hull_of_the_known_values():
    for name in ("disc8", "soup257", "strip200_one_end"):
        r = filled_fixture(name)
        filled = r["level"] >= 1
        known = r["rgb"].astype(np.float64)[r["best"] >= 0]
        assert (r["x0"][filled] >= known.min(axis=0)).all() and (r["x0"][filled] <= known.max(axis=0)).all()
        assert (r["x0"][~filled] == r["rgb"][~filled]).all()


def test_a_ramp_comes_back_as_the_ramp():
    f, rgb, best = fs.plane_ramp()
    ys, xs = np.mgrid[0:fs.NY, 0:fs.NX]
    ramp = (3 * xs + 2 * ys).ravel()
    out, level, st, x, x0 = mf.fill(f, rgb, best)
    unknown = best < 0
    print("ramp: %s; largest |x - ramp| %.3g" % (st, np.abs(x[:, 0] - ramp).max()))
    assert unknown.sum() > 150 and st["filled"] == unknown.sum() and st["clamped"] == 0
    assert np.array_equal(out[:, 0], ramp) and np.array_equal(out[:, 1], ramp + 1) and np.array_equal(out[:, 2], 255 - ramp)
    assert np.abs(x[:, 0] - ramp).max() < 0.05


def test_what_no_known_vertex_reaches_stays_grey():
    f, rgb, best, marks = fs.planted()
    out, level, st, x, x0 = mf.fill(f, rgb, best)
    stay = [marks["loose_unknown"], *marks["island"]]
    assert (level[stay] == -1).all() and (out[stay] == 127).all() and st["unreached"] == 4
    assert (level[best >= 0] == 0).all() and out[best >= 0].tobytes() == rgb[best >= 0].tobytes()
    rest = (best < 0)
    rest[stay] = False
    assert (level[rest] >= 1).all() and st["filled"] == rest.sum() and level.max() == st["rounds"] == 1   # the column and the ring are one edge wide
    assert level.tobytes() == mf.bfs_levels(f, best).tobytes()
    # no known vertex at all, and none unknown: the input's bytes
    for b in (np.full_like(best, -1), np.zeros_like(best)):
        o, lv, s, _, _ = mf.fill(f, rgb, b)
        assert o.tobytes() == rgb.tobytes() and s["filled"] == s["steps"] == 0 and (lv == (b[0] if b[0] < 0 else 0)).all()
    e = np.zeros((0, 3), np.int32)
    o, lv, s, _, _ = mf.fill(e, np.zeros((0, 3), np.uint8), np.zeros(0, np.int32))
    assert o.shape == (0, 3) and lv.shape == (0,) and s["n_vertices"] == 0


def test_given_iterations_and_the_clamp():
    f, rgb, best = fs.soup()
    a = mf.fill(f, rgb, best, iterations=7)
    assert a[2]["steps"] == 7 and a[2]["max_change"] == float(np.abs(a[3] - a[4])[a[1] >= 1].max()) > 0.0
    x0, level, L = mf.front(f, rgb, best)
    assert a[3].tobytes() == mf.solve(f, x0, level, L, 7).tobytes()
    assert mf.solve(f, x0, level, L, 0).tobytes() == x0.tobytes()
    out, n = mf.to_bytes(np.array([[-0.6, 255.5, 12.5], [300.0, -9.0, 1.0]]), np.uint8([[1, 2, 3], [4, 5, 6]]), np.array([True, False]))
    assert out.tolist() == [[0, 255, 13], [4, 5, 6]] and n == 2
