"""CPU replay (oracle only) of the refine data-term cache: the two-way cache (way = key & 1, key = int(d - 1.5)) of one refine
stage as the kernels run it -- k_refine_first with or without its prefill, single sweeps (k_refine_sweep: a miss installs at
once), launches of T sweeps (k_refine_skew, k_refine_tile: a miss installs in the launch's own copy, the first new entry per
pixel and way reaches the cache after the launch) and, before every such launch that starts before sweep REKEY_UNTIL, optionally
the re-key pass (k_refine_rekey).  Used by tests/tools/simulate_rekey.py and tests/test_gpu_refine_miss_service.py."""
import numpy as np

from oracle import oracle as orc

NOMATCH = -10000.0
REKEY_UNTIL = 22  # re-key before the multi-sweep launches that start before this sweep
NONE = -99999


def stage_states(d16, img_own, img_oth, ws, mg, ns):
    """The oracle's states after 0 .. ns sweeps of one refine stage, cut to the interior of margin `mg`, and the pixels whose
    update reads the data term (mode != 0; constant over the sweeps)."""
    states = [d16.astype(np.float64)] + [orc.disparity_refine(d16, img_own, img_oth, n, ws, mg) for n in range(1, ns + 1)]
    YL, YR, XL, XR = mg[0], mg[1], mg[2], mg[3]
    full = states[0]
    sl = (slice(YL + 1, YR), slice(XL + 1, XR))
    c = full[sl] != NOMATCH
    ew = (full[YL + 1:YR, XL + 2:XR + 1] != NOMATCH) & (full[YL + 1:YR, XL:XR - 1] != NOMATCH)
    ns_ = (full[YL + 2:YR + 1, XL + 1:XR] != NOMATCH) & (full[YL:YR - 1, XL + 1:XR] != NOMATCH)
    live = c & (ew | ns_)
    return [s[sl] for s in states], live


def key_of(s):
    return np.trunc(s - 1.5).astype(np.int64)


def nearest_side(s, k):
    v = s - 1.5
    centre = np.where(k > 0, k + 0.5, np.where(k < 0, k - 0.5, 0.0))  # int() truncates: key 0's interval is (-1, 1)
    return np.where(v > centre, k + 1, k - 1)


def simulate(states, live, T, first, policy, nsweeps, prefill=True, on_single=None):
    """Sweeps 1 .. nsweeps - 1 after k_refine_first: launches of T sweeps from sweep `first` on (first >= nsweeps: none), single
    sweeps otherwise.  policy: "today" (no re-key), "near", "dir", "opp" (tools/simulate_rekey.py).  on_single(t, miss) sees the
    miss mask of every single sweep t.  Returns per multi-sweep launch (sweep, misses, rare-row fraction, re-keyed entries)."""
    keys = [key_of(s) for s in states]
    way = [np.full(live.shape, NONE, np.int64), np.full(live.shape, NONE, np.int64)]

    def put(k, sel):
        for b in (0, 1):
            way[b] = np.where(sel & ((k & 1) == b), k, way[b])

    # sweep 0: k_refine_first, its own key and the prefill (the neighbour its update points to)
    k0, rel1 = keys[0], keys[1]
    put(k0, live)
    if prefill:
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
            if on_single:
                on_single(t, miss)
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


def wave_misses(miss, rows_per_wave, cols_per_wave=64):
    """Misses per wave of a kernel whose waves each take cols_per_wave columns x rows_per_wave rows of the interior, from its
    first column and row: an array [wave rows, wave columns]."""
    h, w = miss.shape
    ph, pw = -h % rows_per_wave, -w % cols_per_wave
    m = np.pad(miss, ((0, ph), (0, pw)))
    return m.reshape((h + ph) // rows_per_wave, rows_per_wave, (w + pw) // cols_per_wave, cols_per_wave).sum(axis=(1, 3))
