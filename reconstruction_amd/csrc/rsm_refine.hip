// rsm_refine.hip -- the executor of DisparityRefine's Jacobi sweeps (.cpp:590-678): refine_plan.h decides a level's schedule,
// refine_sweeps walks its steps.  Here are the mechanics alone: the ping-pong buffers, the two launch chains of a split
// section, the event pair of a timed launch, the fork / join events and the turn-taking between the contexts of a GPU.
#include "rsm_ctx.h"

#include <mutex>

// ---- one bandwidth-bound section at a time per GPU ------------------------------------------------------------
// Contexts that share a GPU (rsm_run_pairs / rsm_match_pairs: several pairs in flight) overlap usefully only where
// one of them leaves the chip idle: the launch-latency-bound small levels, the row-serial stages, host syncs.  Two
// pairs' large-level Jacobi sweeps gain nothing from running side by side -- each streams at the fabric's rate
// alone -- and would only halve each other's speed.  So those sections take turns, ordered on the GPU by events (the host
// never blocks for it): a section waits for the event that ends the previous context's section; the short mutex
// only makes "enqueue the section, publish its end event" atomic.
// MEASURED (C2, two pairs in flight): no turns 214-220 Mdisp/s with every top-level sweep launch twice as long (236 us);
// turns for every large level 210 with isolated-like launches (125 us); turns for the TOP level only (the default) 227-231:
// the other pair's second-largest level and full-size non-refine stages then run beside the top-level sweeps and fill
// their launch tails, at the price of 158 us per top-level launch.
// lane 0: sections bound by the fabric (one sweep per launch); lane 1 (option heavy_lanes = 2): the time-skewed sections, bound
// by fp64 issue -- a section of one kind runs well beside a section of the other kind of another pair
static std::mutex g_heavy_mu[RSM_MAX_DEVICES][2];
static hipEvent_t g_heavy_last[RSM_MAX_DEVICES][2];
static rsm_ctx *g_heavy_owner[RSM_MAX_DEVICES][2];

static void heavy_begin(rsm_ctx *c, int lane) { // (whether a section takes turns at all: refine_plan)
    g_heavy_mu[c->device][lane].lock();
    if (g_heavy_last[c->device][lane] && g_heavy_owner[c->device][lane] != c) (void)hipStreamWaitEvent(c->stream, g_heavy_last[c->device][lane], 0);
}
static void heavy_end(rsm_ctx *c, int lane) {
    hipEvent_t ev = lane ? c->ev_heavy2 : c->ev_heavy;
    (void)hipEventRecord(ev, c->stream);
    g_heavy_last[c->device][lane] = ev;
    g_heavy_owner[c->device][lane] = c;
    g_heavy_mu[c->device][lane].unlock();
}
void heavy_forget(rsm_ctx *c) {
    if (c->device >= RSM_MAX_DEVICES) return;
    for (int lane = 0; lane < 2; lane++) {
        std::lock_guard<std::mutex> g(g_heavy_mu[c->device][lane]);
        if (g_heavy_owner[c->device][lane] == c) {
            g_heavy_owner[c->device][lane] = nullptr;
            g_heavy_last[c->device][lane] = nullptr;
        }
    }
}

static RefinePlanIn plan_input(const rsm_ctx *c, const StageArgs &a, int iters, hipStream_t st, bool top, double turn_px) {
    const bool slot = c->device < RSM_MAX_DEVICES; // (a device beyond the tables: never alone, no second chain, no turns)
    RefinePlanIn in{};
    in.W = a.W;
    in.H = a.H;
    in.ndir = a.ndir;
    for (int v = 0; v < a.ndir; v++) in.m[v] = a.d[v].own;
    in.iters = iters;
    in.top = top;
    in.have_upd = a.upd_list != nullptr;
    in.turn_px = slot ? turn_px : 0.0;
    in.skew_from = c->opt_refine_skew_from;
    in.skew_T = c->opt_refine_skew_T;
    in.skew_min_px = c->opt_refine_skew_min_px;
    in.skew_uw = c->opt_refine_skew_uw;
    in.skew_rows = c->opt_refine_skew_rows;
    in.skew_waves = c->opt_refine_skew_waves;
    in.skew_waves_alone = c->opt_refine_skew_waves_alone;
    in.skew_waves_low = c->opt_refine_skew_waves_low;
    in.tile_T = c->opt_refine_tile_T;
    in.tile_from = c->opt_refine_tile_from;
    in.tile_min_px = c->opt_refine_tile_min_px;
    in.rekey_until = c->opt_refine_rekey_until;
    in.split = c->opt_refine_split;
    in.heavy_exclusive = c->opt_heavy_exclusive;
    in.heavy_min_px = c->opt_heavy_min_px;
    in.heavy_from_sweep = c->opt_heavy_from_sweep;
    in.heavy_lanes = c->opt_heavy_lanes;
    in.alone = slot && !c->shared_now() && g_running[c->device].load() == 1;
    in.profiling = c->profile;
    in.second = slot && c->stream2 != st && c->upd_list2;
    return in;
}

// option refine_upd_cap (tests): the update list's shards hold at most that many records
static int capped_upd(const rsm_ctx *c, int cap) { return c->opt_refine_upd_cap > 0 ? std::min(cap, c->opt_refine_upd_cap) : cap; }

// sweeps s.t .. s.t + s.T - 1 as one launch of k_refine_sweep, k_refine_skew or k_refine_tile, a.d[].f64_a -> f64_b
static void launch_step(rsm_ctx *c, StageArgs &a, const RefineStep &s, hipStream_t st) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (s.timed) {
        const int stg = s.launch == RL_SKEW ? ST_REFINE_SKEW_TOP : ST_REFINE_LIGHT_TOP;
        const int es = prof_slot(c, stg);
        e0 = c->evpool[es].a;
        e1 = c->evpool[es].b;
        double bytes = 0; // 16 B per interior pixel and sweep (fp64 in + out)
        for (int v = 0; v < a.ndir; v++) {
            const int r0 = a.d[v].own.YL + 1, r1 = a.d[v].own.YR;
            if (r1 > r0) bytes += 16.0 * (r1 - r0) * (a.d[v].own.XR - a.d[v].own.XL + 1);
        }
        c->prof_launches[stg] += 1;
        c->prof_bytes[stg] += (double)s.T * bytes;
    }
    if (s.launch == RL_SINGLE) {
        launch_refine_sweep(a, st, e0, e1);
        return;
    }
    a.rf_launch = s.rf_launch;
    // one launch chain, or -- a split section -- the two directions as two: one's tail runs beside the other's head
    StageArgs ch[2] = {a, a};
    hipStream_t cs[2] = {st, c->stream2};
    if (s.chains == 2) {
        ch[0].ndir = ch[1].ndir = 1;
        ch[1].d[0] = a.d[1];
        ch[1].upd_list = c->upd_list2;
        ch[1].upd_cnt = c->upd_cnt2;
    }
    // (the previous launch's cache updates are in: k_refine_apply runs behind every multi-sweep launch on the same stream)
    if (s.rekey)
        for (int i = 0; i < s.chains; i++) launch_refine_rekey(ch[i], cs[i]);
    if (s.launch == RL_TILE) launch_refine_tile(a, s.T, st);
    else
        for (int i = 0; i < s.chains; i++) launch_refine_skew(ch[i], s.T, cs[i], i ? nullptr : e0, i ? nullptr : e1); // (e0 / e1 in a split: only under refine_split = 2, an A/B mode)
}

// Sweep t reads A (t even) or B (t odd) and writes the other.
int refine_sweeps(rsm_ctx *c, StageArgs &a, double *const bufA[2], double *const bufB[2], int iters, hipStream_t st, bool top,
                  bool *final_in_B, double turn_px) {
    const RefinePlan plan = refine_plan(plan_input(c, a, iters, st, top, turn_px));
    int launches = 0;
    bool curB = false; // the current values are in bufA
    auto bind = [&]() {
        for (int v = 0; v < a.ndir; v++) {
            a.d[v].f64_a = curB ? bufB[v] : bufA[v];
            a.d[v].f64_b = curB ? bufA[v] : bufB[v];
        }
    };
    for (const RefineStep &s : plan.steps) switch (s.kind) {
        case RS_FIRST:
            bind();
            a.rf_no_prefill = !c->opt_refine_prefill;
            a.rf_rekey_far = c->opt_refine_rekey_side;
            launch_refine_first(a, st);
            launches++;
            curB = true;
            a.upd_cap = capped_upd(c, a.upd_cap);
            if (plan.zero_counters) (void)hipMemsetAsync(a.upd_cnt, 0, sizeof(int32_t) * 2 * RF_UPD_SHARDS, st);
            if (plan.skewT) {
                a.skew_prio = c->opt_refine_skew_prio;
                a.skew_uw = plan.skew_uw;
                a.skew_rows = plan.skew_rows;
            }
            break;
        case RS_TURN_BEGIN: heavy_begin(c, s.lane); break;
        case RS_TURN_END: heavy_end(c, s.lane); break;
        case RS_FORK: // the second stream continues from here
            (void)hipMemsetAsync(c->upd_cnt2, 0, sizeof(int32_t) * 2 * RF_UPD_SHARDS, st);
            (void)hipEventRecord(c->ev_fork, st);
            (void)hipStreamWaitEvent(c->stream2, c->ev_fork, 0);
            break;
        case RS_JOIN:
            (void)hipEventRecord(c->ev_join, c->stream2);
            (void)hipStreamWaitEvent(st, c->ev_join, 0);
            break;
        case RS_LAUNCH:
            bind();
            launch_step(c, a, s, st);
            launches += s.T;
            curB = !curB;
            break;
        }
    *final_in_B = curB;
    return launches;
}

// the one parity entry point that runs the pair path's own scheduler
extern "C" int rsm_stage_refine(rsm_ctx *c, const int16_t *disp_in, const uint8_t *img_own, const uint8_t *img_oth,
                                int W, int H, int iterations, double ws, const rsm_boundary *own, double *disp_out) {
    if (!stage_ok(c, W, H) || !disp_in || !img_own || !img_oth || !own || !disp_out || iterations < 0) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    StageArgs a = one_dir(c, W, H, 0, own, nullptr);
    a.ws = ws;
    DirArgs &d = a.d[0];
    d.d16_in = t.up(disp_in, px);
    d.img_own = t.up(img_own, px * 3);
    d.img_oth = t.up(img_oth, px * 3);
    uint32_t *i4o = t.alloc<uint32_t>(px), *i4t = t.alloc<uint32_t>(px);
    double *A = t.alloc<double>(px), *B = t.alloc<double>(px);
    d.rf_key = t.alloc<uint32_t>(px);
    d.rf_ent = t.alloc<double2>(2 * px);
    a.rf_stride = px;
    a.upd_cap = 4096;
    a.upd_list = t.alloc<RfUpd>((size_t)RF_UPD_SHARDS * a.upd_cap);
    a.upd_cnt = t.alloc<int32_t>(2 * RF_UPD_SHARDS);
    if (!t.ok) return finish(c, t);
    if (iterations > RF_MAX_SWEEPS) return set_err(c, RSM_E_INVALID, "iterations");
    d.f64_a = A;
    d.f64_b = B;
    launch_bgr_to_bgrx(d.img_own, W, H, i4o, c->stream);
    launch_bgr_to_bgrx(d.img_oth, W, H, i4t, c->stream);
    d.img4_own = i4o;
    d.img4_oth = i4t;
    launch_refine_init(a, c->stream);
    double *bufA[2] = {A, nullptr}, *bufB[2] = {B, nullptr};
    bool inB = false;
    refine_sweeps(c, a, bufA, bufB, iterations, c->stream, false, &inB);
    d.f64_a = inB ? B : A; // the buffer the last sweep wrote
    t.down(disp_out, (const double *)d.f64_a, px);
    return finish(c, t);
}
