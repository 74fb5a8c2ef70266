"""CPU simulation (oracle only): the refine data-term cache under re-keying before the early time-skewed launches.

Replays the two-way cache (way = key & 1, key = int(d - 1.5)) of a level's refine as the kernels run it -- k_refine_first
with its prefill, single sweeps (k_refine_sweep: a miss installs at once), time-skewed launches of T sweeps (k_refine_skew:
a miss installs in the launch's LDS copy, the first new entry per pixel and way reaches the cache after the launch) -- and,
before every skewed launch that starts before sweep 22, optionally a re-key pass (k_refine_rekey): the way of the current
key holds that key, the other way holds the predicted neighbour key.  Policies:
  today    no re-key, skewed from sweep 22 (the schedule before this tool)
  near     re-key, neighbour on the side of the interval the state is nearest to
  dir      re-key, neighbour in the direction of the state's last move (ties: nearest side)
  opp      re-key with the side `near` does NOT pick (a deliberately wrong predictor)
For each policy, T and first skewed sweep it prints per skewed launch the misses, the fraction of 64-pixel row segments
(per sweep) with at least one miss -- the rows that take k_refine_skew's rare path -- and the entries the re-key computed.

Usage: python tests/tools/simulate_rekey.py [W H levels]   (default 640 480 5; C2's geometry: 11x11 NCC, offset 2)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from reconstruction_amd import synth  # noqa: E402
from helpers import oracle_stages  # noqa: E402

from refine_cache_replay import REKEY_UNTIL, simulate, stage_states  # noqa: E402

SKEW_FROM_TODAY = 22


def level_states(W, H, N, ns):
    cfg = synth.config_small(W, H, N, radius=5, offset=2, pair=1, holes=False)
    rec, fin = oracle_stages(cfg)
    r = [q for q in rec if q["stage"] == "refine" and q["level"] == N - 1 and q["v"] == 0][0]
    im = fin["imgs"][N - 1]
    return stage_states(r["inp"], im[0], im[1], cfg.ws, r["mg"][0], ns)


def main():
    W, H, N = (int(a) for a in (sys.argv[1:4] + ["640", "480", "5"][len(sys.argv) - 1:]))
    t0 = time.time()
    NS = 34
    states, live = level_states(W, H, N, NS)
    print("# %dx%d, %d levels, top level: %d live interior pixels, %d sweeps simulated (%.0f s)" % (W, H, N, int(live.sum()), NS, time.time() - t0))
    ref = simulate(states, live, 4, SKEW_FROM_TODAY, "today", NS)
    print("today: T 4 from %d -- per launch (sweep, misses, rare-row fraction): %s" % (SKEW_FROM_TODAY, ", ".join("(%d, %d, %.4f)" % r[:3] for r in ref)))
    bar = ref[0][2]
    print("bar: the rare-row fraction of today's first skewed launch = %.4f" % bar)
    print("%-6s %2s %5s | %-s" % ("policy", "T", "first", "per launch before sweep %d: sweep:misses/rare-fraction/re-keyed entries" % REKEY_UNTIL))
    for policy in ("today", "near", "dir", "opp"):
        for T in (2, 3, 4):
            for first in (2, 4, 6, 10):
                rows = simulate(states, live, T, first, policy, NS)
                early = [r for r in rows if r[0] < REKEY_UNTIL]
                worst = max([r[2] for r in early] or [0.0])
                print("%-6s %2d %5d | worst %.4f %s | %s" % (policy, T, first, worst, "ok " if worst <= bar else "---",
                                                           " ".join("%d:%d/%.3f/%d" % r for r in early)))


if __name__ == "__main__":
    main()
