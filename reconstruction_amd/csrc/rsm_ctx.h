// rsm_ctx.h -- what the host units of librsm_mi355.so share: the context, the error helpers and the scoped device
// allocations of an entry point that works on host buffers.  Internal: not installed, not included by include/rsm.h.
#pragma once

#include "../../include/rsm.h"
#include "rsm_dev.h"

#include <atomic>
#include <string>
#include <vector>

// the stages rsm_profile_* accounts for (their names: kStageNames, rsm_api.hip)
enum Stage {
    ST_PYRAMID = 0,
    ST_MARGIN,
    ST_BOXSUM,
    ST_INITIAL_MATCH,
    ST_SMOOTH,
    ST_ORDER,
    ST_UNIQ16,
    ST_REMATCH,
    ST_MEDIAN,
    ST_REFINE_INIT,
    ST_REFINE_SWEEP,     // all levels below the top
    ST_REFINE_SWEEP_TOP, // the top level's sweeps (light + worklist kernels)
    ST_REFINE_LIGHT_TOP, // only the k_refine_sweep<1> launches of the top level
    ST_REFINE_SKEW_TOP,  // only the k_refine_skew<T,1> launches of the top level (T sweeps each; the dominant kernel)
    ST_UNIQ64,
    ST_CLOUD,
    ST_COUNT
};

struct EvPair {
    hipEvent_t a, b;
    int stage;
};

struct rsm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr; // side stream: per-level BGRX copies and window sums (they depend on the images only)
    hipEvent_t ev_pyr = nullptr, ev_prep[RSM_MAX_LEVELS]{};
    std::string err;

    // resident pair
    bool have_pair = false, have_result = false;
    rsm_pair_in in{};
    int N = 0;
    int Wk[RSM_MAX_LEVELS]{}, Hk[RSM_MAX_LEVELS]{};
    uint8_t *img[RSM_MAX_LEVELS][2]{}, *msk[RSM_MAX_LEVELS][2]{};
    Mg mg[RSM_MAX_LEVELS][2]{};
    int h_margin_init[RSM_MAX_LEVELS * 2 * 4]{}; // host source of the margins' initial values (async copy)

    // workspace (sized for the top level)
    size_t cap_px = 0;
    std::vector<void *> allocs;
    int *d_margins = nullptr; // N*2*4 ints
    int32_t *S1[RSM_MAX_LEVELS][2]{}, *S2[RSM_MAX_LEVELS][2]{}, *tmp1 = nullptr, *tmp2 = nullptr; // per level and view
    uint32_t *img4[RSM_MAX_LEVELS][2]{};
    int16_t *d16a[2]{}, *BL[2]{}, *BR[2]{}; // d16a: scratch (Rectify's mask temp)
    uint8_t *cloud_flags = nullptr;         // k_cloud's per-pixel "emitted a point" flags of the last run: rsm_filter_last_cloud's lattice reads them
                                            // long after rsm_run_pair has returned, so they have a buffer nothing else borrows
    int16_t *d16i[RSM_MAX_LEVELS][2]{}, *d16s[RSM_MAX_LEVELS][2]{}, *d16m[RSM_MAX_LEVELS][2]{}; // per level: initial-match / constraint-stage / median maps, pre-filled NOMATCH
    double *f64[3][2]{};
    int32_t *nv[2]{};
    uint32_t *rf_key[2]{};
    int32_t *rf_cnt = nullptr; // NCC wide-pixel counter
    int32_t *wrow = nullptr;   // NCC: wide pixels per (direction, row) of the level at hand
    uint32_t *rf_list = nullptr;
    uint32_t *tie_list = nullptr; // NCC tie pixels (k_ncc_exact)
    int32_t *tie_cnt = nullptr;   // [2 * level + (Rematch ? 1 : 0)]
    double2 *rf_ent[2]{};
    RfUpd *upd_list = nullptr; // k_refine_skew's cache updates
    int32_t *upd_cnt = nullptr;
    int upd_cap = 0;
    int32_t *prefix = nullptr;
    int *d_j1 = nullptr, *d_j2 = nullptr;   // structuring-element spans: Rectify's mask erosion
    int *d_cj1 = nullptr, *d_cj2 = nullptr; // ... and DisparityToCloud's (uploaded with the pair)
    uint8_t *blk = nullptr;                 // coarse bad-block map of the top-level mask (cloud erosion)
    hipEvent_t ev_cloudprep = nullptr;
    int ordinal = 0;               // n-th context created on its device
    int opt_cu_share = 0;          // > 1: the context's streams are confined to one of that many equal shares of the compute units
    hipEvent_t ev_heavy = nullptr; // end of this context's last bandwidth-bound section (heavy_begin / heavy_end)
    hipStream_t stream_filter = nullptr; // rsm_filter_last_cloud's stream: the lowest priority the device offers (filter_stream())
    hipEvent_t ev_filter = nullptr;      // orders the filter behind whatever `stream` still holds
    hipEvent_t ev_heavy2 = nullptr; // ... of its last issue-bound (time-skewed) section: lane 1
    hipEvent_t ev_fork = nullptr, ev_join = nullptr; // the two directions of a time-skewed section on two streams (refine_sweeps)
    RfUpd *upd_list2 = nullptr;     // the second direction's update list / counters while the two run as separate launch chains
    int32_t *upd_cnt2 = nullptr;
    int opt_refine_split = 1;       // a pair that has the GPU to itself runs the two directions of its time-skewed sections on two streams
    int opt_shared_gpu = 0;         // the caller's hint that other contexts use this GPU (a pool of pairs in flight): never split, whatever g_running says at the moment
    int pool_shared = 0;            // the same, derived per call by rsm_run_pairs / rsm_match_pairs from their pool (the caller's option stays as set)
    bool shared_now() const { return opt_shared_gpu || pool_shared; }
    std::atomic<int> in_run{0};     // inside rsm_run_pair (options that replace the streams refuse to act then)
    int32_t *row_count = nullptr;
    int64_t *row_offset = nullptr;
    int64_t *d_npoints = nullptr;
    unsigned long long *d_vtop = nullptr;
    double *d_q = nullptr, *d_R = nullptr, *d_T = nullptr;
    double *xyz = nullptr;
    uint8_t *bgr = nullptr;
    rsm_point16 *pack16 = nullptr; // the cloud as 16-byte records / the filter's output, staged for a host download (on first use)
    float *pack_nrm = nullptr;     // ... and the filter's normals
    FilterArena *filt_arena = nullptr; // the cloud filter's scratch (created on first use, grows with the cloud)
    PoissonMesh pmesh;                 // the last mesh of rsm_poisson_mesh / rsm_stage_iso_mesh (rsm_poisson_last_mesh copies it out)
    uint8_t *mcol_rgb = nullptr;       // rsm_mesh_color_last's colours of that mesh (rsm_mesh_last_colors copies them out) ...
    int32_t *mcol_best = nullptr;      // ... and best views
    bool mcol_valid = false;           // they are the colours of pmesh as it is now: a later mesh has none (mesh_replaced())
    long long opt_meshcolor_big_box = 4096; // rsm_mesh_color: a (face, view) bounding box of more pixels is strided by a block, not walked by one thread
    int opt_filter_wg_max = 2048;      // rsm_filter_last_cloud: the wave passes' workgroup form while at most this many queries are left (0: never)
    int opt_filter_normals_window = 8; // rsm_filter_last_cloud: the normals' radius search on the pixel lattice while no point needs a wider window than this (0: grid)
    int filt_normals[2]{};             // last rsm_filter_last_cloud: the window the normals used (0: the grid), the widest a point needed (-1: not asked)
    int opt_filter_list = 23;          // ... and the 24-pixel window a thread each for what the tile pass leaves over
    int filt_memo_radius = 0, filt_memo_k = 0, filt_memo_w = 0, filt_memo_h = 0, filt_memo_uses = 0; // rsm_filter_last_cloud: the last probe's choice
    int opt_filter_low_priority = 1;   // rsm_filter_last_cloud on a stream of the lowest priority (1) or on the context's own (0)
    int opt_filter_window = 1;         // rsm_filter_last_cloud: the pixel-window k-nearest pass in front of the grid ladder (1: radius from a sparse probe; 0: off; else the radius)
    int64_t filt_tile_left = 0;        // ... queries the tile pass alone left over
    int64_t filt_info[4]{};            // last rsm_filter_last_cloud: window pass used, queries it left to the ladder, points in, points kept
    FilterPasses filt_passes;          // last rsm_filter_last_cloud / rsm_stage_filter_depth_map: the wave passes, the ladder, the whole-cloud search (rsm_filter_last_passes)
    FilterRoute filt_route;            // the grid ladder: option "filter_ladder_h" in, what the last rsm_filter_cloud / rsm_filter_last_cloud did out;
                                       // .outrem: the radius outlier pass's setting (rsm_filter_set_outrem) in, its report (rsm_filter_last_outrem) out

    // results
    double *res_disp[2]{};
    int64_t n_points = 0;
    int64_t v_top = 0;

    // options (rsm_set_option)
    int opt_ncc_bytes = 0;
    int opt_no_exact = 0;
    int opt_no_rowgemm = 0;
    int opt_ncc_mid = 0;         // rows that hold many (RG_MIN) pixels with intervals longer than this go to a row kernel; 0 = by window size
                                 // (measured crossover against the band kernel: 11x11 from ~40 candidates on, 5x5 beyond 160)
    int opt_ncc_slide_max = 512; // rows whose widest interval has at most this many candidates take the sliding-sums kernel, the others the int8 row GEMM
    int opt_heavy_from_sweep = 1;  // ... from this sweep of the level on
    int opt_heavy_min_px = 400000; // ... from this many margin pixels on (smaller levels are launch-bound themselves)
    int opt_heavy_lanes = 2;     // 2: the single-sweep part and the time-skewed part of a level's refine take turns separately (lanes 0 / 1)
    int opt_heavy_exclusive = 1; // refine sections of contexts sharing a GPU take turns (heavy_begin): 1 = the top level's, 2 = every large level's, 0 = none
    int opt_refine_skew_from = 4;  // first sweep of a level that may run in the time-skewed kernel (k_refine_skew; 0: never): 22 without the re-key below -- before
                                   // that too many pixels still miss the data-term cache for its lane-serial miss service
    int opt_refine_rekey_until = 22; // a time-skewed launch that starts before this sweep is preceded by k_refine_rekey (both cache ways set for the current
                                     // state: the key and its nearer neighbour), which keeps the early launches' misses at the settled rate (0: never)
    int opt_refine_rekey_side = 0;   // 1: k_refine_rekey installs the FARTHER neighbour (a wrong prediction: tests)
    int opt_refine_prefill = 1;    // k_refine_first also fills the second cache way with the neighbour iMatch its update points to
    int opt_refine_skew_T = 4;     // sweeps per time-skewed launch (2..4)
    int opt_refine_skew_min_px = 1000000; // ... at levels with at least this many margin pixels per direction (smaller levels: the 4T-step pipeline fill of a chunk eats the gain)
    int opt_refine_skew_waves = 2560;    // workgroups a time-skewed launch aims at (sets the rows per chunk): 5 per CU are resident, so two rounds --
                                         // workgroups at different points of their chunks share a CU better than 1 280 in lockstep (measured: 0.28 against 0.34 ms)
    int opt_refine_skew_waves_alone = 3840; // ... when no other context of the device is inside rsm_run_pair (0: the same)
    int opt_refine_skew_waves_low = 640; // ... at the levels below the top while other contexts are inside rsm_run_pair (0: the same as the top's): taller chunks
                                         // recompute fewer halo rows, which is what the other pairs' kernels pay for (C2 in flight: 386 -> 394 Mdisp/s)
    int opt_refine_skew_rows = 0;        // > 0: rows per chunk, overrides refine_skew_waves (tests)
    int opt_refine_skew_prio = 0;        // the time-skewed kernel's waves rotate their issue priority every 2^this shader clocks (0: never)
    int opt_refine_skew_uw = 0;          // columns a strip owns; 0: 66 - 2T, all its last level can compute (an even number <= that: A/B)
    int opt_refine_tile_T = 4;           // sweeps per launch of the tile kernel (k_refine_tile; 2..RF_TILE_MAXT, 0: off) at the levels below refine_skew_min_px
    int opt_refine_tile_from = 4;        // ... from this sweep of a level on (k_refine_rekey in front of the launches before refine_rekey_until)
    int opt_refine_tile_min_px = 0;      // ... at levels with at least this many margin pixels per direction
    int opt_refine_upd_cap = 0;          // > 0: the update list's shards hold at most this many records (tests: overflow costs misses, never bits)

    // what the last rsm_stage_initial_match's NCC launch decided (rsm_stage_last_ncc_routes): its per-row counters and row
    // lists (StageArgs::wrow, rsm_dev.h), the worklist length and the tie count; H = 0 until such a call succeeded
    std::vector<int32_t> ncc_wit_wrow;
    int ncc_wit_H = 0;
    int32_t ncc_wit_cnt = 0, ncc_wit_ties = 0;

    // profiling
    bool profile = false;
    bool profile_stages = false;
    std::vector<EvPair> evpool;
    size_t ev_used = 0;
    double prof_ms[ST_COUNT]{};
    int64_t prof_launches[ST_COUNT]{};
    double prof_bytes[ST_COUNT]{};
};

int set_err(rsm_ctx *c, int code, const char *fmt, ...); // rsm_api.hip
int prof_slot(rsm_ctx *c, int stage);                    // rsm_api.hip: the next event pair of the pool, booked to `stage`

// contexts inside rsm_run_pair, per device: a pair that finds itself alone there schedules its refine differently (refine_plan.h)
#define RSM_MAX_DEVICES 64
inline std::atomic<int> g_running[RSM_MAX_DEVICES];
struct RunningGuard {
    int dev;
    std::atomic<int> *own;
    RunningGuard(int d, std::atomic<int> *in_run) : dev(d), own(in_run) {
        if (dev < RSM_MAX_DEVICES) g_running[dev].fetch_add(1);
        own->store(1);
    }
    ~RunningGuard() {
        own->store(0);
        if (dev < RSM_MAX_DEVICES) g_running[dev].fetch_sub(1);
    }
};

// rsm_refine.hip: the executor of a level's refine schedule.  Returns the number of sweeps launched; *final_in_B tells which
// buffer holds the result.  turn_px: margin pixels per direction for the turn-taking with the device's other contexts (0: none).
int refine_sweeps(rsm_ctx *c, StageArgs &a, double *const bufA[2], double *const bufB[2], int iters, hipStream_t st, bool top,
                  bool *final_in_B, double turn_px = 0.0);
void heavy_forget(rsm_ctx *c); // the context goes away: nobody may wait on its turn events any more

#define HIPCHK(c, call)                                                                               \
    do {                                                                                              \
        hipError_t e__ = (call);                                                                      \
        if (e__ != hipSuccess)                                                                        \
            return set_err((c), RSM_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__),    \
                           __FILE__, __LINE__);                                                       \
    } while (0)

static inline Mg to_mg(const rsm_boundary &b) { return Mg{b.YL, b.YR, b.XL, b.XR}; }
static inline rsm_boundary to_boundary(const Mg &m) {
    return rsm_boundary{m.YL, m.YR, m.XL, m.XR, m.XR - m.XL + 1, m.YR - m.YL + 1};
}
static inline bool degenerate(const Mg &m) { return m.YL >= m.YR || m.XL >= m.XR; } // .cpp:827
void ellipse_spans(int k, std::vector<int> &j1, std::vector<int> &j2); // rsm_api.hip

template <typename T>
static int dalloc(rsm_ctx *c, T **p, size_t n) {
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, n * sizeof(T) + 64);
    if (e != hipSuccess) return set_err(c, RSM_E_NOMEM, "hipMalloc(%zu) failed: %s", n * sizeof(T), hipGetErrorString(e));
    c->allocs.push_back(q);
    *p = (T *)q;
    return RSM_OK;
}

struct Tmp { // scoped device allocations of one stage call
    rsm_ctx *c;
    std::vector<void *> ptrs;
    bool ok = true;
    hipError_t down_err = hipSuccess; // the first later() copy that failed: finish() names it
    bool pending = false; // an up() copy may still be reading its host buffer: no wait for c->stream since
    explicit Tmp(rsm_ctx *c_) : c(c_) {}
    ~Tmp() {
        if (pending) (void)hipStreamSynchronize(c->stream); // an early return: the caller's buffers are free again once it has returned
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    T *alloc(size_t n) {
        void *p = nullptr;
        if (hipMalloc(&p, n * sizeof(T) + 64) != hipSuccess) {
            ok = false;
            return nullptr;
        }
        ptrs.push_back(p);
        return (T *)p;
    }
    // The copy is only enqueued: finish(), down() or at the latest the destructor waits for it, so h must outlive this Tmp or
    // the call's finish().  n = 0 allocates and copies nothing (h may be NULL).  nullptr: no device memory; a copy that failed
    // clears `ok`, which finish() reports.
    template <typename T>
    T *up(const T *h, size_t n) {
        T *d = alloc<T>(n);
        if (d && n > 0) {
            if (hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, c->stream) != hipSuccess) ok = false;
            pending = true;
        }
        return d;
    }
    // n elements down where there are any and the caller gave room for them; only enqueued: finish() waits and reports a failure
    template <typename T>
    Tmp &later(T *h, const T *d, size_t n) {
        if (n > 0 && h && down_err == hipSuccess) down_err = hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, c->stream);
        return *this;
    }
    template <typename T>
    void down(T *h, const T *d, size_t n) {
        if (hipMemcpyAsync(h, d, n * sizeof(T), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            ok = false;
        pending = false;
    }
};
static inline int finish(rsm_ctx *c, Tmp &t) {
    hipError_t e = hipStreamSynchronize(c->stream);
    t.pending = false;
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return set_err(c, RSM_E_HIP, "stage failed: %s", hipGetErrorString(e));
    if (t.down_err != hipSuccess) return set_err(c, RSM_E_HIP, "hipMemcpyAsync (device to host) failed: %s", hipGetErrorString(t.down_err));
    if (!t.ok) return set_err(c, RSM_E_HIP, "stage alloc/copy failed");
    return RSM_OK;
}
// ---- what the mesh units' entries share (rsm_poisson.hip, rsm_mesh.hip) ---------------------------------------------------------------------
// the end of the *_fail texts: after a HIP failure ": " and the runtime's last error, else nothing
static inline std::string hip_tail(int s) { return s == RSM_E_HIP ? std::string(": ") + hipGetErrorString(hipGetLastError()) : std::string(); }
// The colours of rsm_mesh_color_last / rsm_mesh_stitch_last are those of the mesh they were computed on.  Whoever hands &c->pmesh to a producer
// calls this once the producer has replaced (or freed) that mesh; nothing else decides whether the colours still hold.
static inline void mesh_replaced(rsm_ctx *c) { c->mcol_valid = false; }

static inline bool stage_ok(rsm_ctx *c, int W, int H) { return c && W > 0 && H > 0 && hipSetDevice(c->device) == hipSuccess; }

// the arguments of a one-direction stage call on host buffers (the parity entry points)
static inline StageArgs one_dir(rsm_ctx *c, int W, int H, int r, const rsm_boundary *own, const rsm_boundary *oth) {
    StageArgs a{};
    a.opt_ncc_bytes = c->opt_ncc_bytes;
    a.opt_no_exact = c->opt_no_exact;
    a.opt_no_rowgemm = c->opt_no_rowgemm;
    a.ncc_mid = c->opt_ncc_mid;
    a.ncc_slide_max = c->opt_ncc_slide_max;
    a.ndir = 1;
    a.W = W;
    a.H = H;
    a.r = r;
    a.d[0].own = to_mg(*own);
    if (oth) a.d[0].oth = to_mg(*oth);
    return a;
}
