"""The refine schedule (csrc/refine_plan.h) on the CPU: tests/cpp/refine_plan_dump.cpp, built with plain g++, prints the plan
of every case below; each must equal what the pair path enqueued before the schedule became a plan
(tests/refine_schedule_restatement.py), and each must have the properties a schedule needs whatever produced it."""
import itertools
import os
import subprocess

import pytest

from refine_schedule_restatement import FIELDS, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PX = 90 * 60  # margin pixels per direction of the base level below: the *_min_px thresholds are set on both sides of it
BASE = dict(W=96, H=64, ndir=2, YL0=2, YR0=61, XL0=3, XR0=92, YL1=2, YR1=61, XL1=3, XR1=92, iters=33, top=1, have_upd=1, turn_px=PX,
            skew_from=4, skew_T=4, skew_min_px=PX, skew_uw=0, skew_rows=0, skew_waves=2560, skew_waves_alone=3840, skew_waves_low=640,
            tile_T=4, tile_from=4, tile_min_px=0, rekey_until=22, split=1, heavy_exclusive=1, heavy_min_px=0, heavy_from_sweep=1,
            heavy_lanes=2, alone=1, profiling=0, second=1)
assert sorted(BASE) == sorted(FIELDS)


def product(**sets):
    keys = list(sets)
    for vals in itertools.product(*(sets[k] for k in keys)):
        yield dict(zip(keys, vals))


def margins(kind, W, H=64):
    """Both directions' margins of a W x 64 level: inside (the skew kernel fits), touching row 0 or the last column (it does not),
    an interior of 0 rows, and two directions of different widths."""
    m = dict(inside=(2, H - 3, 3, W - 4), row0=(0, H - 3, 3, W - 4), lastcol=(2, H - 3, 3, W - 1), norows=(7, 8, 3, W - 4),
             uneven=(2, H - 3, 9, W - 20))[kind]
    first = (2, H - 3, 3, W - 4) if kind == "uneven" else m
    return dict(zip(("YL0", "YR0", "XL0", "XR0", "YL1", "YR1", "XL1", "XR1"), first + m))


def cases():
    out = []
    # which kernel a sweep goes to, the re-key in front, the counter sets: every threshold of the sweep index
    for v in product(iters=(0, 1, 2, 5, 30, 33, 150), skew_T=(2, 3, 4), skew_from=(0, 1, 4, 22), tile_T=(0, 2, 4, 8), tile_from=(1, 4),
                     rekey_until=(0, 3, 22), skew_min_px=(PX, PX + 1)):
        out.append(dict(BASE, **v))
    # the level's constants: strip width, rows per chunk, whether the skew kernel fits the level at all
    for v in product(W=(79, 80), kind=("inside", "row0", "lastcol", "norows", "uneven"), ndir=(1, 2), skew_uw=(0, 40, 62), skew_T=(2, 3, 4),
                     skew_rows=(0, 16), waves=((2560, 3840, 640), (1, 0, 0), (100, 0, 7), (64, 5, 0)), alone=(0, 1), top=(0, 1)):
        w = dict(zip(("skew_waves", "skew_waves_alone", "skew_waves_low"), v.pop("waves")))
        out.append(dict(BASE, skew_min_px=0, W=v["W"], **margins(v.pop("kind"), v.pop("W")), **w, **v))
    # fork / join and the turns
    for v in product(ndir=(1, 2), alone=(0, 1), split=(0, 1, 2), profiling=(0, 1), second=(0, 1), heavy_exclusive=(0, 1, 2), top=(0, 1),
                     heavy_lanes=(1, 2), heavy_from_sweep=(1, 10, 1000)):
        out.append(dict(BASE, turn_px=PX + 0.5, **v))  # (the mean of two directions' pixel counts may end in .5)
    # turns without a time-skewed section, on both sides of heavy_min_px, for a caller that never takes turns, without an update list
    for v in product(turn_px=(0, PX), heavy_min_px=(PX, PX + 1), iters=(5, 33), skew_from=(0, 22), tile_T=(0, 4), tile_min_px=(PX, PX + 1),
                     heavy_exclusive=(1, 2), heavy_lanes=(1, 2), heavy_from_sweep=(1, 10, 1000), top=(0, 1), have_upd=(0, 1)):
        out.append(dict(BASE, skew_min_px=PX + (v["skew_from"] == 0), **v))
    return out


def parse(line):
    tok = line.split()
    return tuple(int(x) for x in tok[:4]), tok[4:]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = tmp_path_factory.mktemp("refine_plan") / "refine_plan_dump"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I" + os.path.join(ROOT, "reconstruction_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "refine_plan_dump.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cs = cases()
    text = "".join(" ".join(repr(c[f]) for f in FIELDS) + "\n" for c in cs)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cs)
    return cs, [parse(l) for l in lines]


def test_the_cases_straddle_the_thresholds(plans):
    """The case list reaches what it is meant to reach: every kind of step and launch, both answers of every level decision."""
    cs, got = plans
    assert 2000 <= len(cs) <= 20000
    seen = set()
    for (skewT, uw, rows, zero), steps in got:
        seen.update(s[:3] if s[0] == "L" else s[0] for s in steps)
        seen.add("skew" if skewT else "noskew")
        seen.add("zero%d" % zero)
        seen.update("chains2" for s in steps if s[0] == "L" and s.split(":")[6] == "2")
        seen.update("timed" for s in steps if s[0] == "L" and s.split(":")[7] == "1")
        seen.update("rekey" for s in steps if s[0] == "L" and s.split(":")[5] == "1")
    assert seen >= {"F", "B", "E", "K", "J", "L:S", "L:W", "L:T", "skew", "noskew", "zero0", "zero1", "chains2", "timed", "rekey"}


def test_plan_equals_the_schedule_the_pair_path_enqueued(plans):
    cs, got = plans
    for c, g in zip(cs, got):
        want = schedule(c)
        assert g == (tuple(want[0]), want[1]), c


def test_every_plan_is_a_sound_schedule(plans):
    """Stated without the restatement.  The level constants of a level that does not skew are not used and stay 0; where it does,
    the kernel's limits hold: a strip's columns are even in number (or all 66 - 2T the last sweep can compute) and at most 66 - 2T,
    a chunk has at least a row."""
    cs, got = plans
    for c, ((skewT, uw, rows, zero), steps) in zip(cs, got):
        iters = c["iters"]
        if iters <= 0:
            assert not steps and (skewT, uw, rows, zero) == (0, 0, 0, 0), c
            continue
        assert steps[0] == "F" and steps.count("F") == 1, c
        if skewT:
            assert skewT == c["skew_T"] and (uw % 2 == 0 or uw == 66 - 2 * skewT) and 0 < uw <= 66 - 2 * skewT and rows >= 1, c
        else:
            assert uw == 0 and rows == 0, c
        takes_turns = c["turn_px"] > 0 and c["heavy_exclusive"] != 0 and c["turn_px"] >= c["heavy_min_px"] and (c["heavy_exclusive"] == 2 or c["top"])
        t, nmulti, forked, held = 1, 0, False, {0: False, 1: False}
        for s in steps[1:]:
            if s[0] == "L":
                kind, st, T, rf, rekey, chains, timed = [x if i == 0 else int(x) for i, x in enumerate(s.split(":")[1:])]
                assert st == t, c  # the launches cover the sweeps 1 .. iters - 1 in order, each once
                t += T
                if kind == "S":
                    assert T == 1 and rf == -1 and rekey == 0 and chains == 1, c
                else:
                    frm, TT = (c["skew_from"], c["skew_T"]) if kind == "W" else (c["tile_from"], c["tile_T"])
                    assert T == TT and st >= frm and st + T <= iters, c
                    assert kind == "T" or skewT, c
                    assert zero == 1, c  # the counters a multi-sweep launch appends to were zeroed
                    assert rf == nmulti, c
                    nmulti += 1
                    assert rekey == int(st < c["rekey_until"]), c
                assert chains == (2 if forked else 1), c
                assert not (forked and kind != "W"), c  # a fork is joined before the next launch that is not time-skewed
                assert not timed or (c["profiling"] and c["top"] and kind != "T"), c
            elif s == "K":
                assert not forked and c["ndir"] == 2 and c["second"] and c["split"], c
                forked = True
            elif s == "J":
                assert forked, c
                forked = False
            else:
                lane = int(s[1])
                assert takes_turns and s[0] in "BE", c
                assert held[lane] == (s[0] == "E"), c  # begin and end alternate on a lane
                assert not (s[0] == "E" and forked), c  # ... and a turn ends only behind the join
                held[lane] = s[0] == "B"
        assert t == iters and not forked and not held[0] and not held[1], c
