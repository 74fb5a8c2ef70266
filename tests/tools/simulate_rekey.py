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

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as orc  # noqa: E402
from reconstruction_amd import synth  # noqa: E402
from helpers import oracle_stages  # noqa: E402

NOMATCH = -10000.0
SKEW_FROM_TODAY = 22
REKEY_UNTIL = 22  # re-key before the skewed launches that start before this sweep
NONE = -99999


def level_states(W, H, N, ns):
    cfg = synth.config_small(W, H, N, radius=5, offset=2, pair=1, holes=False)
    rec, fin = oracle_stages(cfg)
    r = [q for q in rec if q["stage"] == "refine" and q["level"] == N - 1 and q["v"] == 0][0]
    d16, mg = r["inp"], r["mg"][0]
    im = fin["imgs"][N - 1]
    states = [d16.astype(np.float64)] + [orc.disparity_refine(d16, im[0], im[1], n, cfg.ws, mg) for n in range(1, ns + 1)]
    YL, YR, XL, XR = mg[0], mg[1], mg[2], mg[3]
    full = states[0]
    sl = (slice(YL + 1, YR), slice(XL + 1, XR))
    c = full[sl] != NOMATCH
    ew = (full[YL + 1:YR, XL + 2:XR + 1] != NOMATCH) & (full[YL + 1:YR, XL:XR - 1] != NOMATCH)
    ns_ = (full[YL + 2:YR + 1, XL + 1:XR] != NOMATCH) & (full[YL:YR - 1, XL + 1:XR] != NOMATCH)
    live = c & (ew | ns_)  # the pixels whose update reads the data term (mode != 0); constant over the sweeps
    return [s[sl] for s in states], live


def key_of(s):
    return np.trunc(s - 1.5).astype(np.int64)


def nearest_side(s, k):
    v = s - 1.5
    centre = np.where(k > 0, k + 0.5, np.where(k < 0, k - 0.5, 0.0))  # int() truncates: key 0's interval is (-1, 1)
    return np.where(v > centre, k + 1, k - 1)


def simulate(states, live, T, first, policy, nsweeps):
    keys = [key_of(s) for s in states]
    way = [np.full(live.shape, NONE, np.int64), np.full(live.shape, NONE, np.int64)]

    def put(k, sel):
        for b in (0, 1):
            way[b] = np.where(sel & ((k & 1) == b), k, way[b])

    # sweep 0: k_refine_first, its own key and the prefill (the neighbour its update points to)
    k0, rel1 = keys[0], keys[1]
    put(k0, live)
    rel2 = np.where(rel1 != k0, rel1, np.where(states[1] > states[0], k0 + 1, np.where(states[1] < states[0], k0 - 1, k0)))
    put(rel2, live & (np.abs(rel2 - k0) == 1))
    W = live.shape[1]
    nseg = (W + 63) // 64
    pad = nseg * 64 - W
    rows = []
    t, prev = 1, 0
    while t < nsweeps:
        skew = t >= first and t + T <= nsweeps
        if not skew:
            k = keys[t]
            miss = live & (np.where(k & 1, way[1], way[0]) != k)
            put(k, miss)
            prev, t = t, t + 1
            continue
        rk = 0
        if policy != "today" and t < REKEY_UNTIL:
            k, s = keys[t], states[t]
            near = nearest_side(s, k)
            if policy == "near":
                p = near
            elif policy == "opp":
                p = 2 * k - near
            else:
                p = np.where(s > states[prev], k + 1, np.where(s < states[prev], k - 1, near))
            own = live & (np.where(k & 1, way[1], way[0]) != k)
            oth = live & (np.where(p & 1, way[1], way[0]) != p)
            rk = int(own.sum() + oth.sum())
            put(k, own)
            put(p, oth)
        lds = [way[0].copy(), way[1].copy()]
        first_new = [np.full(live.shape, NONE, np.int64), np.full(live.shape, NONE, np.int64)]
        nm = nrare = 0
        for s_ in range(T):
            k = keys[t + s_]
            miss = live & (np.where(k & 1, lds[1], lds[0]) != k)
            for b in (0, 1):
                sel = miss & ((k & 1) == b)
                first_new[b] = np.where(sel & (first_new[b] == NONE), k, first_new[b])
                lds[b] = np.where(sel, k, lds[b])
            nm += int(miss.sum())
            seg = np.pad(miss, ((0, 0), (0, pad))).reshape(miss.shape[0], nseg, 64).any(axis=2)
            nrare += int(seg.sum())
        for b in (0, 1):
            way[b] = np.where(first_new[b] != NONE, first_new[b], way[b])
        rows.append((t, nm, nrare / float(T * live.shape[0] * nseg), rk))
        prev, t = t, t + T
    return rows


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
