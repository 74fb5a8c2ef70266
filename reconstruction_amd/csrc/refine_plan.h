// refine_plan.h -- the schedule of one level's DisparityRefine sweeps as data: which sweeps run one per launch, time-skewed
// or on tiles, which launches get a re-key in front, when the two directions fork onto the second stream, when the section
// takes its turn against the other contexts of the GPU, which launches are timed.  Plain C++ (nothing of HIP): the executor
// (refine_sweeps, rsm_refine.hip) walks the steps and decides nothing; tests/cpp/refine_plan_dump.cpp prints them.
#pragma once

#include <algorithm>
#include <vector>

// Margin of one view at one level (struct Boundary, CManageData.h:10-14, without width/height).
struct Mg {
    int YL, YR, XL, XR;
};

// interior rows / columns of the margins, the largest over the directions: what a refine launch's grid covers; false: nothing to do
inline bool refine_interior(const Mg *m, int ndir, int &rows, int &cols) {
    rows = cols = 0;
    for (int v = 0; v < ndir; v++) {
        if (m[v].YR - m[v].YL - 1 > rows) rows = m[v].YR - m[v].YL - 1;
        if (m[v].XR - m[v].XL - 1 > cols) cols = m[v].XR - m[v].XL - 1;
    }
    return rows > 0 && cols > 0;
}

// strips of 64 lanes the interior of margin m takes in k_refine_skew (strip b owns the columns [xorg + T - 1 + b uw, + uw) of
// [XL + 1, XR - 1])
inline int refine_skew_strips(const Mg &m, int T, int uw) {
    const int xorg = (m.XL + 1 - (T - 1)) & ~7;
    return std::max(1, (m.XR - xorg - T + 1 + uw - 1) / uw);
}

// k_refine_skew addresses rows of 64 + 4 columns on the flat row-major buffers without clamping: a strip may hang over a row's
// ends into the neighbouring rows, never out of the level (rows 1 .. H - 2 are the only ones a margin can hold, r >= 1).
inline bool refine_skew_fits(int W, int H, const Mg *m, int ndir) {
    if (W < 80 || H < 3) return false;
    for (int v = 0; v < ndir; v++)
        if (m[v].XL < 1 || m[v].YL < 1 || m[v].XR > W - 2 || m[v].YR > H - 2) return false;
    return true;
}

struct RefinePlanIn {
    int W, H, ndir; // the level; m[0 .. ndir - 1] its margins
    Mg m[2];
    int iters;       // sweeps, the first one included
    bool top;        // the pyramid's top level
    bool have_upd;   // an update list exists (the multi-sweep kernels need one)
    double turn_px;  // margin pixels per direction that the turn-taking weighs against heavy_min_px; 0: the caller never takes turns
    // options (rsm_set_option), as stored
    int skew_from, skew_T, skew_min_px, skew_uw, skew_rows, skew_waves, skew_waves_alone, skew_waves_low;
    int tile_T, tile_from, tile_min_px;
    int rekey_until, split;
    int heavy_exclusive, heavy_min_px, heavy_from_sweep, heavy_lanes;
    // the facts of the moment
    bool alone;     // no other context of the device is inside rsm_run_pair, and none was announced (shared_gpu, a pool)
    bool profiling; // rsm_profile_enable is on
    bool second;    // a second stream and a second update list exist: the two directions can run as two launch chains
};

enum RefineStepKind { RS_FIRST, RS_TURN_BEGIN, RS_TURN_END, RS_FORK, RS_JOIN, RS_LAUNCH };
enum RefineLaunchKind { RL_SINGLE, RL_SKEW, RL_TILE }; // k_refine_sweep (T = 1), k_refine_skew, k_refine_tile

struct RefineStep {
    RefineStepKind kind;
    int lane = 0;                     // TURN_BEGIN / TURN_END: 0 the single-sweep sections (fabric-bound), 1 the time-skewed ones (fp64 issue)
    RefineLaunchKind launch = RL_SINGLE; // LAUNCH: sweeps t .. t + T - 1
    int t = 0, T = 0;
    int rf_launch = -1;               // index among the level's multi-sweep launches (picks the update list's counter set); -1: a single sweep
    bool rekey = false;               // k_refine_rekey in front
    int chains = 1;                   // 2: the two directions as two launch chains on the two streams
    bool timed = false;               // bracketed by a profiling event pair
};

struct RefinePlan {
    int skewT = 0;     // > 0: the level has a time-skewed section of skewT sweeps per launch, and the two constants below hold
    int skew_uw = 0;   // columns a strip owns
    int skew_rows = 0; // rows per chunk
    bool zero_counters = false; // the update list's counters are zeroed behind the first sweep (a multi-sweep kernel may run)
    std::vector<RefineStep> steps; // in enqueue order
};

// Sweep 0 is k_refine_first (every pixel computes its data term); then one launch per sweep while the data-term cache fills,
// and from sweep `skew_from` on the large levels run skew_T sweeps per launch, time-skewed, the levels below them tile_T
// sweeps per launch on overlapped tiles from `tile_from` on; leftover sweeps run single again.
inline RefinePlan refine_plan(const RefinePlanIn &in) {
    RefinePlan p;
    if (in.iters <= 0) return p;
    p.steps.reserve((size_t)in.iters + 12); // a launch per sweep at most, one fork / join, the lanes change hands twice at most
    auto step = [&](RefineStepKind kind, int lane = 0) {
        RefineStep s{};
        s.kind = kind;
        s.lane = lane;
        p.steps.push_back(s);
    };
    step(RS_FIRST);
    double px = 0;
    for (int v = 0; v < in.ndir; v++) px += (double)(in.m[v].XR - in.m[v].XL + 1) * (in.m[v].YR - in.m[v].YL + 1);
    // settled sweeps of the large levels T per launch, time-skewed (k_refine_skew)
    const bool skew = in.skew_from > 0 && in.have_upd && px / in.ndir >= in.skew_min_px && refine_skew_fits(in.W, in.H, in.m, in.ndir);
    const int skewT = skew ? in.skew_T : 0;
    // the levels below that: T sweeps per launch on overlapped tiles (k_refine_tile) -- they are bound by launch latency
    const bool tile = in.tile_T >= 2 && in.have_upd && px / in.ndir < in.skew_min_px && px / in.ndir >= in.tile_min_px;
    const int tileT = tile ? in.tile_T : 0;
    p.zero_counters = skew || tile;
    if (skew) {
        p.skewT = skewT;
        p.skew_uw = (in.skew_uw > 0 && in.skew_uw <= 66 - 2 * skewT) ? in.skew_uw : 66 - 2 * skewT;
        int rows, cols, strips = 0;
        refine_interior(in.m, in.ndir, rows, cols);
        rows = std::max(rows, 1);
        for (int v = 0; v < in.ndir; v++) strips += refine_skew_strips(in.m[v], skewT, p.skew_uw);
        // A pair that has the GPU to itself takes twice as many, half as tall chunks: its launches end in a tail of one or two
        // waves per SIMD that nothing else fills, and a second round of workgroups shortens it; with pairs in flight the other
        // pairs' kernels fill the tail and the extra pipeline fill only costs.
        const bool lone = in.alone && in.skew_waves_alone > 0;
        // Below the top level, with pairs in flight, the aim has a value of its own (skew_waves_low): there the launch's
        // own time matters less than the work it costs the other pairs' kernels, and taller chunks recompute fewer halo rows.
        const int waves = lone ? in.skew_waves_alone : ((!in.top && in.skew_waves_low > 0) ? in.skew_waves_low : in.skew_waves);
        const int chunks = std::max(1, waves / std::max(1, strips));
        p.skew_rows = in.skew_rows > 0 ? in.skew_rows : std::max(4 * skewT, (rows + chunks - 1) / chunks);
    }
    // The section that takes turns with the other contexts of this GPU starts once the sweeps have settled into pure
    // streaming: the first ones are busy computing data terms (VALU) and run well beside another pair's streaming sweeps.
    // heavy_exclusive 1: only the top level's sweeps take turns, 2: every large level's.
    const bool turns = in.turn_px > 0.0 && in.heavy_exclusive && in.turn_px >= (double)in.heavy_min_px && (in.heavy_exclusive != 1 || in.top);
    const int turn_from = in.turn_px > 0.0 ? std::min(std::max(in.heavy_from_sweep, 1), in.iters) : in.iters + 1;
    // A pair that has the GPU to itself (and no per-launch timing) runs the two directions of a time-skewed section as separate
    // launch chains on its two streams: every skewed launch ends in a tail of one or two waves per SIMD, and the other
    // direction's launch fills it.  With pairs in flight the other pairs' kernels do that already, and the split costs
    // throughput (measured): not used there.  split = 2 forces it (A/B).
    const bool may_split = skew && in.ndir == 2 && in.split && (!in.profiling || in.split == 2) && in.second && (in.split == 2 || in.alone);
    bool held = false, split_now = false;
    int lane = 0, nmulti = 0, ntimed = 0;
    auto join = [&]() {
        if (split_now) step(RS_JOIN);
        split_now = false;
    };
    auto turn_end = [&]() {
        if (held) step(RS_TURN_END, lane);
        held = false;
    };
    for (int t = 1; t < in.iters;) {
        const bool skew_now = skew && t >= in.skew_from && t + skewT <= in.iters;
        if (!skew_now) join(); // (before the lane is handed on: the section's end event must cover the second stream's launches)
        if (in.heavy_lanes == 2 && (int)skew_now != lane && t >= turn_from) { // the section changes kind: hand its lane on
            turn_end();
            lane = (int)skew_now;
        }
        if (turns && t >= turn_from && !held) {
            step(RS_TURN_BEGIN, lane);
            held = true;
        }
        if (skew_now && may_split && !split_now) { // behind TURN_BEGIN's wait on the main stream, so the second direction takes turns like the first
            step(RS_FORK);
            split_now = true;
        }
        const bool tile_now = tile && t >= in.tile_from && t + tileT <= in.iters;
        RefineStep s{};
        s.kind = RS_LAUNCH;
        s.launch = skew_now ? RL_SKEW : (tile_now ? RL_TILE : RL_SINGLE);
        s.t = t;
        s.T = skew_now ? skewT : (tile_now ? tileT : 1);
        s.timed = in.profiling && in.top && s.launch != RL_TILE && (ntimed++ & 7) == 4; // every 8th sweep launch of the top level
        if (s.launch != RL_SINGLE) {
            s.rf_launch = nmulti++;
            s.rekey = t < in.rekey_until; // an early launch: both cache ways are first set for the state it starts from
            s.chains = (s.launch == RL_SKEW && split_now) ? 2 : 1;
        }
        p.steps.push_back(s);
        t += s.T;
    }
    join();
    turn_end();
    return p;
}
