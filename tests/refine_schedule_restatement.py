"""The refine schedule as the pair path enqueued it before it became a plan: `refine_sweeps` of csrc/rsm_api.hip at commit
4f0d0b9 (lines 514-649) with `heavy_begin` / `heavy_end` (lines 55-69), transcribed statement by statement -- the decisions
only; where that code enqueued something, this appends a step.  tests/test_refine_plan_cpu.py holds csrc/refine_plan.h to it.

A case is a dict of the fields FIELDS names (the inputs of RefinePlanIn).  The three facts of the moment stand for
    alone     = c->device < RSM_MAX_DEVICES && !c->shared_now() && g_running[c->device].load() == 1      (:600, :617)
    profiling = c->profile                                                                              (:538, :616)
    second    = c->stream2 != st && c->upd_list2 && c->device < RSM_MAX_DEVICES                          (:616-617)
and turn_px for the caller's heavy_px (0 from rsm_stage_refine, :1081; Pk from rsm_run_pair, :810; heavy_begin's own
`c->device >= RSM_MAX_DEVICES` (:56) is a turn_px of 0 as well: no section of such a context ever took a turn).
"""

FIELDS = ("W H ndir YL0 YR0 XL0 XR0 YL1 YR1 XL1 XR1 iters top have_upd turn_px "
          "skew_from skew_T skew_min_px skew_uw skew_rows skew_waves skew_waves_alone skew_waves_low "
          "tile_T tile_from tile_min_px rekey_until split heavy_exclusive heavy_min_px heavy_from_sweep heavy_lanes "
          "alone profiling second").split()


def cdiv(a, b):
    """C's integer division (truncation towards zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def skew_strips(m, T, uw):  # k_refine_skew.hip:448-451
    xorg = (m["XL"] + 1 - (T - 1)) & ~7
    return max(1, cdiv(m["XR"] - xorg - T + 1 + uw - 1, uw))


def skew_fits(W, H, margins):  # k_refine_skew.hip:455-462
    if W < 80 or H < 3:
        return False
    for m in margins:
        if m["XL"] < 1 or m["YL"] < 1 or m["XR"] > W - 2 or m["YR"] > H - 2:
            return False
    return True


def interior(margins):  # rsm_dev.h:123-131
    rows = cols = 0
    for m in margins:
        rows = max(rows, m["YR"] - m["YL"] - 1)
        cols = max(cols, m["XR"] - m["XL"] - 1)
    return rows, cols


def schedule(c):
    """-> (constants, steps): constants = (skewT, skew_uw, skew_rows, counters zeroed), steps = the dump program's tokens."""
    margins = [dict(YL=c["YL%d" % v], YR=c["YR%d" % v], XL=c["XL%d" % v], XR=c["XR%d" % v]) for v in range(c["ndir"])]
    iters, top, ndir = c["iters"], bool(c["top"]), c["ndir"]
    steps = []
    state = dict(nlaunch=0, nmulti=0, split_now=False)

    def heavy_begin(lane):  # :55-61
        if not c["heavy_exclusive"] or c["turn_px"] < float(c["heavy_min_px"]):
            return False
        if c["heavy_exclusive"] == 1 and not top:
            return False
        steps.append("B%d" % lane)
        return True

    def heavy_end(held, lane):  # :62-69
        if held:
            steps.append("E%d" % lane)

    def launch(t, kind, T):  # :536-571
        timed = False
        if c["profiling"] and top and kind != "T":  # :538 (nlaunch++ only where the tests before it hold)
            timed = (state["nlaunch"] & 7) == 4
            state["nlaunch"] += 1
        rf, rekey, nch = -1, 0, 1
        if kind != "S":  # :549-568
            rf = state["nmulti"]
            state["nmulti"] += 1
            nch = 2 if (kind == "W" and state["split_now"]) else 1  # :552
            rekey = int(t < c["rekey_until"])  # :563
        steps.append("L:%s:%d:%d:%d:%d:%d:%d" % (kind, t, T, rf, rekey, nch, int(timed)))

    if iters <= 0:  # :573
        return (0, 0, 0, 0), steps
    px = 0.0
    for m in margins:  # :575
        px += float(m["XR"] - m["XL"] + 1) * (m["YR"] - m["YL"] + 1)
    steps.append("F")  # :579
    skew = c["skew_from"] > 0 and bool(c["have_upd"]) and px / ndir >= c["skew_min_px"] and skew_fits(c["W"], c["H"], margins)  # :583
    skewT = c["skew_T"] if skew else 0
    tile = c["tile_T"] >= 2 and bool(c["have_upd"]) and px / ndir < c["skew_min_px"] and px / ndir >= c["tile_min_px"]  # :586
    tileT = c["tile_T"] if tile else 0
    zero = int(skew or tile)  # :589
    uw = rows_per_chunk = 0
    if skew:  # :590-606
        uw = c["skew_uw"] if (0 < c["skew_uw"] <= 66 - 2 * skewT) else 66 - 2 * skewT
        rows, _ = interior(margins)
        rows = max(rows, 1)
        strips = sum(skew_strips(m, skewT, uw) for m in margins)
        lone = bool(c["alone"]) and c["skew_waves_alone"] > 0  # :600
        if lone:  # :603
            waves = c["skew_waves_alone"]
        elif not top and c["skew_waves_low"] > 0:
            waves = c["skew_waves_low"]
        else:
            waves = c["skew_waves"]
        chunks = max(1, cdiv(waves, max(1, strips)))
        rows_per_chunk = c["skew_rows"] if c["skew_rows"] > 0 else max(4 * skewT, cdiv(rows + chunks - 1, chunks))  # :605
    held, lane = False, 0
    turn_from = min(max(c["heavy_from_sweep"], 1), iters) if c["turn_px"] > 0.0 else iters + 1  # :611
    may_split = (skew and ndir == 2 and c["split"] != 0 and (not c["profiling"] or c["split"] == 2) and bool(c["second"])
                 and (c["split"] == 2 or bool(c["alone"])))  # :616-617

    def join():  # :618-623
        if state["split_now"]:
            steps.append("J")
            state["split_now"] = False

    t = 1
    while t < iters:  # :624-644
        skew_now = skew and t >= c["skew_from"] and t + skewT <= iters
        if not skew_now:
            join()
        if c["heavy_lanes"] == 2 and int(skew_now) != lane and t >= turn_from:
            heavy_end(held, lane)
            held = False
            lane = int(skew_now)
        if t >= turn_from and not held:
            held = heavy_begin(lane)
        if skew_now and may_split and not state["split_now"]:
            steps.append("K")
            state["split_now"] = True
        tile_now = tile and t >= c["tile_from"] and t + tileT <= iters
        T = skewT if skew_now else (tileT if tile_now else 1)
        launch(t, "W" if skew_now else ("T" if tile_now else "S"), T)
        t += T
    join()  # :645
    heavy_end(held, lane)  # :646
    return (skewT, uw, rows_per_chunk, zero), steps
