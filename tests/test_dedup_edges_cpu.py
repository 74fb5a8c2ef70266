"""The duplicate deletion's edge fixtures (tests/dedup_edge_fixtures.py) on the CPU: the numpy restatement
(tests/dedup_restatement.py) and the independent bucket-list statement (tests/dedup_bucket_lists.py) agree on every fixture; every
fixture reaches what it claims to reach (counted from these two statements, never from the kernel); CurrentValue agrees with a
plain numpy correlation wherever it is read; and the restatement with one rule changed disagrees on a named fixture, so the
fixtures can tell that rule.  tests/test_gpu_dedup_edges.py runs the same fixtures through csrc/k_dedup.hip.

Out of scope (see dedup_edge_fixtures.py): the 64-bit key instantiation, the open Eigen reduction-order question, and the bounds the
entry refuses."""
import functools
import inspect

import numpy as np
import pytest

import dedup_bucket_lists as bl
import dedup_edge_fixtures as fx
import dedup_restatement as dr

F = np.float32


@functools.lru_cache(maxsize=None)
def lists(name):
    """(indices, stats, trace) of the bucket-list statement, once per fixture."""
    xyz, nrm, views = fx.get(name)
    tr = {}
    with np.errstate(all="ignore"):
        idx, st = bl.dedup(xyz, nrm, views, tr)
    return idx, st, tr


def restated(name, dedup=None):
    xyz, nrm, views = fx.get(name)
    with np.errstate(all="ignore"):
        return (dedup or dr.dedup)(xyz, nrm, views)


def agrees(name, dedup=None):
    try:
        idx, st = restated(name, dedup)
    except IndexError:              # a changed rule that leaves an image or a bucket: it does not agree
        assert dedup is not None
        return False
    ridx, rst, _ = lists(name)
    return np.array_equal(idx, ridx) and st == rst


@pytest.mark.parametrize("name", list(fx.FIXTURES))
def test_the_two_statements_agree(name):
    idx, st = restated(name)
    ridx, rst, _ = lists(name)
    assert np.array_equal(idx, ridx), (len(idx), len(ridx))
    assert st == rst
    assert idx.dtype == np.int32 and ridx.dtype == np.int32


def plain_ncc(view, X, Y):
    def vec(img):
        u = img[Y - 2:Y + 3, X - 2:X + 3, :].astype(np.float64).ravel()
        u = u - u.mean()
        n = np.sqrt(np.dot(u, u))
        return u, (1.0 if n == 0 else n)
    (a, na), (b, nb) = vec(view["image"][0]), vec(view["image"][1])
    return float(np.dot(a, b)) / (nb * na)


@pytest.mark.parametrize("name", list(fx.FIXTURES))
def test_current_value_against_a_plain_correlation(name):
    views = fx.get(name)[2]
    for (i, X, Y), cv in lists(name)[2]["cv"].items():
        assert abs(cv - plain_ncc(views[i], X, Y)) <= 1e-13, (i, X, Y, cv)


# ---- what each fixture reaches ----------------------------------------------------------------------------------------------------
def test_minus_one_reaches_all_three_classes():
    xyz, nrm, views = fx.get("minus_one")
    idx, st, tr = lists("minus_one")
    assert views[0]["bound"][4] * views[0]["bound"][5] == 936 and st["visited"] == 2 * 936
    sizes = {(i, X, Y): len(m) for i, X, Y, m in tr["buckets"]}
    assert all(sizes[k] == (2 if k[0] == 0 else 3) for k in sizes) and len(tr["cv"]) == 2 * 936
    for pair in (0, 1):
        cv = np.array([v for (i, X, Y), v in tr["cv"].items() if i == pair])
        eq, gt, lt = int((cv == -1).sum()), int((cv > -1).sum()), int((cv < -1).sum())
        print("minus_one pair %d: CurrentValue == -1 at %d, > -1 at %d, < -1 at %d pixels" % (pair, eq, gt, lt))
        assert eq >= 100 and gt >= 100 and lt >= 100
        near = cv[np.abs(cv + 1) < 1e-9]
        assert len(near) >= 600 and np.abs(near + 1).max() <= 4.5e-16       # the last bit decides
    assert tr["cv"][(0, 8, 8)] == 0.0                                       # the flat block: both norms 0
    fl, rn = fx.MINUS_ONE_FLAT, fx.MINUS_ONE_RANDOM
    assert fl[0].start + 2 <= 8 < fl[0].stop - 2 and -0.9 < tr["cv"][(0, rn[1].start + 4, rn[0].start + 4)] < 0.9
    # the value decides every bucket: pair 0 keeps its first point, pair 1 the depth-10 point instead of the farthest
    kept = set(idx.tolist())
    for i, X, Y, m in tr["buckets"]:
        above = tr["cv"][(i, X, Y)] > -1
        if i == 0:
            assert [j in kept for j in m] == [above, False]
        else:
            assert [j in kept for j in m] == [above, False, not above]
    assert st["count0"] == 936


def _dist32(p, C):
    d = [F(p[k]) - F(C[k]) for k in range(3)]
    with np.errstate(all="ignore"):
        return np.sqrt(bl.dot3(d, d))


def test_exhaustive_patterns_has_every_case_once_and_visited():
    xyz, nrm, views = fx.get("exhaustive_patterns")
    v = views[0]
    idx, st, tr = lists("exhaustive_patterns")
    cases = fx.exhaustive_cases()
    buckets = {(X, Y): m for i, X, Y, m in tr["buckets"]}
    assert len(buckets) == len(tr["buckets"]) == len(cases) == 8 + 3 * (64 + 256 + 1024) == st["visited"]
    R1, T1 = bl._rt(v["P"][1])
    seen = set()
    classes = dict(eq=0, gt=0, lt=0)
    for c in cases:
        m = buckets[c["pixel"]]
        assert len(m) == c["size"]
        C = np.asarray(v["C"], np.float64)
        dirs = tuple(bool(np.dot(nrm[j, :3].astype(np.float64), xyz[j].astype(np.float64) - C) < 0) for j in m)
        rights = []
        for j in m:
            x, y = bl.project(R1, T1, xyz[j])
            rights.append(bool(0 <= x < 96 and 0 <= y < 64 and v["mask"][1][y, x] == 255))
        assert dirs == tuple(c["dirs"]) and tuple(rights) == tuple(c["rights"])
        if c["size"] == 2:
            assert (bl.dot3(nrm[m[0]], nrm[m[1]]) < 0) == c["opposite"]
            key = (2, c["opposite"], tuple(rights))
        else:
            order = tr["order"][(0,) + c["pixel"]]
            d = [_dist32(xyz[j], v["C"]) for j in m]
            if c["layout"] == "ascending":
                assert order == list(range(c["size"]))[::-1] and all(d[k] < d[k + 1] for k in range(c["size"] - 1))
            elif c["layout"] == "descending":
                assert order == list(range(c["size"])) and all(d[k] > d[k + 1] for k in range(c["size"] - 1))
            else:
                a, b = c["tie"]
                assert a < b and d[a] == d[b] and xyz[m[a]][2] != xyz[m[b]][2]
                assert order.index(b) == order.index(a) + 1                 # equal distances keep bucket order
                assert len(set(float(t) for t in d)) == c["size"] - 1
            key = (c["size"], dirs, tuple(rights), c["layout"])
        assert key not in seen
        seen.add(key)
        cv = dr.current_value(v, *c["pixel"])
        classes["eq" if cv == -1 else "gt" if cv > -1 else "lt"] += 1
    assert len(seen) == len(cases)
    print("exhaustive_patterns: %d cases; CurrentValue classes %s" % (len(cases), classes))
    assert min(classes.values()) >= 500
    ties = {(c["size"],) + c["tie"] for c in cases if c["layout"] == "equal"}
    assert len(ties) == 3 + 6 + 10                                          # every pair of positions ties somewhere


def test_exhaustive_extremes_buckets():
    xyz, nrm, views = fx.get("exhaustive_extremes")
    idx, st, tr = lists("exhaustive_extremes")
    E = fx.EXTREME_PIXELS
    b = {(X, Y): m for i, X, Y, m in tr["buckets"]}
    assert {k: len(b[E[k]]) for k in E} == dict(big=2000, alternating=300, infinite5=5, infinite3=3, centre=4, infinite4=4)
    C = views[0]["C"]
    d = lambda k: [float(_dist32(xyz[j], C)) for j in b[E[k]]]    # noqa: E731
    assert [np.isinf(t) for t in d("infinite5")] == [False, True, False, True, False]
    assert tr["order"][(0,) + E["infinite5"]][:2] == [1, 3]                 # equal (infinite) distances keep bucket order
    assert [np.isinf(t) for t in d("infinite3")] == [True, False, True] and tr["order"][(0,) + E["infinite3"]] == [0, 2, 1]
    assert sum(np.isinf(t) for t in d("infinite4")) == 1
    assert d("centre")[1] == 0.0 and d("centre")[3] == 0.0 and tr["order"][(0,) + E["centre"]] == [2, 0, 1, 3]
    # the 300-point bucket alternates direction along the distance order: one run per member, all but the nearest emitted
    o = tr["order"][(0,) + E["alternating"]]
    m = b[E["alternating"]]
    dirs = [nrm[m[k]][2] < 0 for k in o]
    assert all(dirs[k] != dirs[k + 1] for k in range(299))
    kept = set(idx.tolist())
    assert sum(j in kept for j in m) == 299 and m[o[-1]] not in kept
    assert len(set(d("big"))) == 2000


@pytest.mark.parametrize("variant", list(fx.SORTED_VARIANTS))
def test_sorted_array_edges_positions(variant):
    nv, extra, starts = fx.SORTED_VARIANTS[variant]
    xyz, nrm, views = fx.get("sorted_" + variant)
    idx, st, tr = lists("sorted_" + variant)
    assert len(xyz) == nv + extra and st["s1"] + st["s2"] == extra and sum(o >= 0 for o in tr["owner"]) == nv
    pos, found = 0, []
    for i, X, Y, m in tr["buckets"]:           # visiting order is key order: the sorted array
        if len(m) > 1:
            found.append((pos, len(m)))
        pos += len(m)
    assert pos == nv and tuple(found) == tuple(starts)
    for s, size in starts:
        crosses = [b for b in (64, 256) if s < b < s + size]
        assert crosses or s + size in (64, 256, nv) or s in (256,), (s, size)


def test_sorted_variants_cover_the_issue_s_sizes():
    V = fx.SORTED_VARIANTS.values()
    assert {v[0] for v in V} == {0, 1, 255, 256, 257, 512}
    assert {1, 255, 256, 257} <= {v[0] + v[1] for v in V}
    starts = {s for v in V for s, _ in v[2]}
    assert {62, 63, 254, 255, 256} <= starts and any(s == v[0] - 3 for v in V for s, _ in v[2])
    assert {3, 5} == {z for v in V for _, z in v[2]}


@pytest.mark.parametrize("total", [4095, 4096, 4097])
def test_key_totals(total):
    xyz, nrm, views = fx.get("total_%d" % total)
    idx, st, tr = lists("total_%d" % total)
    assert sum(v["bound"][4] * v["bound"][5] for v in views) == total
    assert bin(4096).count("1") == 1
    occupied = {(i, X, Y) for i, X, Y, m in tr["buckets"]}
    for i, v in enumerate(views):
        YL, YR, XL, XR, w, h = v["bound"]
        assert (i, XL, YL) in occupied and (i, XR, YR) in occupied          # the first and the last key of each pair
    assert st["s1"] == 0 and st["visited"] == 8


def test_near_ties_counts():
    xyz, nrm, views = fx.get("near_ties")
    idx, st, tr = lists("near_ties")
    v = np.array([[float(t) for t in r] for r in tr["values"]], np.float32)
    assert np.all(v > 0.5)
    gap = np.abs(v[:, 0].view(np.int32).astype(np.int64) - v[:, 1].view(np.int32))
    ties, one_ulp = int((gap == 0).sum()), int((gap == 1).sum())
    first, second = int((v[:, 0] >= v[:, 1]).sum()), int((v[:, 0] < v[:, 1]).sum())
    print("near_ties: %d exact ties, %d one ulp apart, %d further; pair 0 wins %d (%d strictly), pair 1 wins %d"
          % (ties, one_ulp, int((gap > 1).sum()), first, int((v[:, 0] > v[:, 1]).sum()), second))
    assert ties >= 500 and one_ulp >= 500 and int((v[:, 0] > v[:, 1]).sum()) >= 200 and second >= 200
    # the chosen pair shows: pair 1's left mask is 0 (s2), pair 0's 255 (bucketed)
    assert st["s2"] == second and st["s1"] == 0 and sum(o == 0 for o in tr["owner"]) == first
    assert set(idx.tolist()) <= {j for j in range(len(xyz)) if tr["owner"][j] == 0}


def test_rounding_lands_where_double_puts_it():
    xyz, nrm, views = fx.get("rounding")
    idx, st, tr = lists("rounding")
    v = views[0]
    X0, Y0 = fx.ROUNDING_HALF_PIXEL
    b = {(X, Y): m for i, X, Y, m in tr["buckets"]}
    R1, T1 = bl._rt(v["P"][1])
    kept = set(idx.tolist())
    assert tr["cv"][(0, X0, Y0)] > -1
    for t, dpt in enumerate(fx.ROUNDING_RIGHT_DEPTHS):
        m = b[(X0 + t, Y0)]
        assert len(m) == 2 and xyz[m[0]][2] == F(dpt) and xyz[m[1]][2] == 1.0
        col = bl.round_(F(dpt))
        inside = col is not None and 0 <= col < 30 and col % 2 == 0
        assert (m[0] in kept) == inside and m[1] not in kept, dpt
    j = b[(X0, Y0)][0]
    q = xyz[j][2]
    assert q == F(0.49999997) and float(q) == 0.5 - 2.0 ** -25
    assert bl.project(R1, T1, xyz[j]) == (0, 0) and int(q + F(0.5)) == 1     # double: column 0; float q + 0.5f: column 1
    assert v["mask"][1][0, 0] == 255 and v["mask"][1][1, 1] == 0 and j in kept
    cols = {d: bl.round_(F(d)) for d in fx.ROUNDING_RIGHT_DEPTHS}
    assert cols[-0.5] == 0 and cols[-1.5] == -1 and cols[-1.4999999] == 0 and cols[-1.5000001] == -1
    assert cols[2.0 ** 31] is None and cols[-(2.0 ** 31)] == -2147483647 and cols[-2147483904.0] is None and cols[2147483520.0] == 2147483520
    # the left view: k + 0.5 and its upper neighbour land on k + 1, the lower neighbour on k
    occupied = set(b)
    for k, row in ((5, 4), (6, 7), (20, 10)):
        assert {(k, row), (k + 1, row + 1), (k + 1, row + 2)} <= occupied
    for k, col in ((7, 24), (8, 27), (21, 30)):
        assert {(col, k), (col + 1, k + 1), (col + 2, k + 1)} <= occupied
    assert st["s1"] == 30 and st["s2"] == 0            # the negative, huge, non-finite, z = 0 and z < 0 quotients, and only they


@pytest.mark.parametrize("variant", list(fx.UNEQUAL_VARIANTS))
def test_unequal_pairs_reach_the_rims(variant):
    xyz, nrm, views = fx.get("unequal_" + variant)
    idx, st, tr = lists("unequal_" + variant)
    empty = fx.UNEQUAL_VARIANTS[variant]
    assert len({v["mask"][0].shape for v in views}) == 4 and len({tuple(v["bound"]) for v in views}) == 4
    per_pair = len(xyz) // 4
    assert st["s1"] == 4 * (4 - len(empty)) + per_pair * len(empty)
    occupied = {(i, X, Y) for i, X, Y, m in tr["buckets"]}
    cols, rows, left_values = set(), set(), set()
    for i, ((W, H), (YL, YR, XL, XR)) in enumerate(zip(fx.UNEQUAL_SIZES, fx.UNEQUAL_BOUNDS)):
        if i in empty:
            assert not any(o == i for o in tr["owner"])
            continue
        assert {(i, XL, YL), (i, XR, YL), (i, XL, YR), (i, XR, YR)} <= occupied
        R1, T1 = bl._rt(views[i]["P"][1])
        for j in range(len(xyz)):
            if tr["owner"][j] == i:
                x, y = bl.project(R1, T1, xyz[j])
                cols.add(("W" if x == W else "W-1" if x == W - 1 else x) if i % 2 == 0 else None)
                rows.add(("H" if y == H else "H-1" if y == H - 1 else y) if i % 2 == 1 else None)
        for j in range(len(xyz)):
            X, Y = [bl.round_(xyz[j][k] / xyz[j][2]) for k in range(2)]
            if XL <= X <= XR and YL <= Y <= YR and abs(float(np.dot(nrm[j, :3], fx.toward(xyz[j], fx.FAR_CENTRES[i])[:3])) - 1) < 1e-6:
                left_values.add(int(views[i]["mask"][0][Y, X]))
    if len(empty) < 4:
        if any(i % 2 == 0 and i not in empty for i in range(4)):
            assert {-1, 0, "W-1", "W"} <= cols
        if any(i % 2 == 1 and i not in empty for i in range(4)):
            assert {-1, 0, "H-1", "H"} <= rows
        assert left_values == {0, 1, 254, 255}
    else:
        assert len(idx) == 0 and st == dict(s1=len(xyz), s2=0, count0=0, visited=0)
    if variant == "full":
        # the last pixel of one pair and the first of the next are both occupied: neighbouring keys across a pair's end
        assert st["visited"] == 20 and st["s2"] == 4
        assert fx.UNEQUAL_BOUNDS[0][0] == 2 and fx.UNEQUAL_BOUNDS[0][3] == fx.UNEQUAL_SIZES[0][0] - 3   # windows at 0 and W - 5


# ---- one rule changed at a time ---------------------------------------------------------------------------------------------------
def with_source(old, new, count=1):
    """dedup_restatement.dedup with one piece of its text replaced (compiled here, never written anywhere)."""
    src = inspect.getsource(dr.dedup)
    assert src.count(old) == count, (old, src.count(old))
    ns = dict(vars(dr))
    exec(compile(src.replace(old, new), "<changed restatement>", "exec"), ns)
    return ns["dedup"]


def float_round(q):
    v = (np.asarray(q, np.float32) + np.float32(0.5)).astype(np.float64)
    ok = (v > -2147483649.0) & (v < 2147483648.0)
    r = np.zeros(v.shape, np.int64)
    r[ok] = np.trunc(v[ok]).astype(np.int64)
    return ok, r


def single_accumulator_value(view, X, Y):
    """CurrentValue with one running sum per reduction instead of Armadillo's two."""
    def vec(img):
        u = np.ascontiguousarray(img[Y - 2:Y + 3, X - 2:X + 3, :]).reshape(-1).astype(np.float64)
        return [t - float(u.sum()) / len(u) for t in u]          # (the byte sum is exact either way)

    def acc(a, b):
        s = 0.0
        for x, y in zip(a, b):
            s += x * y
        return s
    a, b = vec(view["image"][0]), vec(view["image"][1])
    na, nb = np.sqrt(acc(a, a)), np.sqrt(acc(b, b))
    return acc(a, b) / ((1.0 if nb == 0 else nb) * (1.0 if na == 0 else na))


SORT_LINE = "srt = sorted(good, key=lambda l: -float(d[l])) + [l for l in range(len(bucket)) if not d[l] > 0]"
RULES = {
    # rule: (how to change the restatement, the fixture that must then disagree with the bucket-list statement)
    "float q + 0.5f": (lambda mp: mp.setattr(dr, "_round", float_round), "rounding"),
    "<= in the best-pair comparison": (lambda mp: with_source("upd = best < val", "upd = best <= val"), "near_ties"),
    "sort unstable for equal distances": (lambda mp: with_source("key=lambda l: -float(d[l])", "key=lambda l: (-float(d[l]), -l)"),
                                          "exhaustive_patterns"),
    "zero-distance candidates first": (lambda mp: with_source(
        SORT_LINE, "srt = [l for l in range(len(bucket)) if not d[l] > 0] + sorted(good, key=lambda l: -float(d[l]))"), "exhaustive_extremes"),
    "l != size - 1 dropped": (lambda mp: with_source(" and l != len(bucket) - 1", ""), "exhaustive_patterns"),
    "the nearest point emitted": (lambda mp: with_source(
        "                last = l\n", "                last = l\n            out.append(bucket[srt[-1]])\n"), "exhaustive_patterns"),
    ">= -1": (lambda mp: with_source("if value() > mx:", "if value() > mx or (mx == -1.0 and value() == -1.0):", 2), "minus_one"),
    "single-accumulator NCC": (lambda mp: mp.setattr(dr, "current_value", single_accumulator_value), "minus_one"),
    "pair 0's width for every pair": (lambda mp: with_source(
        "        X, Y = (k - bases[i]) % w + XL", "        w = int(views[0][\"bound\"][4]); X, Y = (k - bases[i]) % w + XL"), "unequal_full"),
}


@pytest.mark.parametrize("rule", list(RULES))
def test_a_changed_rule_is_caught(rule, monkeypatch):
    change, fixture = RULES[rule]
    assert agrees(fixture)
    changed = change(monkeypatch)            # a new dedup, or None when a helper of the module was patched
    assert not agrees(fixture, changed), "%s: not told apart by %s" % (rule, fixture)


def test_base_look_up_without_the_empty_pair_test_is_the_same_rule():
    """'Empty pairs not skipped in the base look-up' cannot be told apart by any input: an empty pair's base equals the base of the
    next pair that owns buckets (or the key total, above every key, when none follows), and the look-up takes the LAST pair whose
    base is <= the key, so the owner always wins over the empty pairs before it.  Dropping the test changes nothing; the kernel's
    `P[t].bw > 0 && P[t].bh > 0` and the restatement's `bases[t] is not None` are redundant.  This holds that on the variants with
    an empty first pair and an empty pair between two owners (test_dedup_cpu.py and random_scene have the empty last pair)."""
    keep_all = with_source("bases.append(base if (w > 0 and h > 0) else None)", "bases.append(base)")
    for name in ("unequal_empty_first", "unequal_empty_middle", "unequal_full"):
        assert agrees(name, keep_all)
    xyz, nrm, views = fx.get("unequal_empty_middle")
    bases, base = [], 0
    for v in views:
        bases.append(base)
        if v["bound"][4] > 0 and v["bound"][5] > 0:
            base += v["bound"][4] * v["bound"][5]
    assert bases[2] == bases[3] and bases[0] == 0                # the empty pair shares its successor's base
