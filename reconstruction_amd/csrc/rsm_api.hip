// rsm_api.hip -- host side of librsm_mi355.so: context, per-pair pipeline and the C ABI of include/rsm.h.
//
// Pipeline = CStereoMatching::MatchAllLayer loop body (reconstruction/CStereoMatching.cpp:21-29) from the
// rectified top-level images: ConstructPyrm (:1040-1053) -> MatchOneLayer x PyrmNum (:36-113, stage order
// kept exactly) -> DisparityToCloud<double> (:682-761).  Everything stays resident in HBM between the one
// upload and the one download; both matching directions run in the same launches (gridDim.z).
#include "rectify_host.h"
#include "rsm_ctx.h"

#include <algorithm>
#include <thread>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const char *kStageNames[ST_COUNT] = {"pyramid", "margin", "boxsum", "initial_match", "smooth", "order",
                                            "uniqueness_s16", "rematch", "median", "refine_init",
                                            "refine_sweep", "refine_sweep_top", "refine_light_top", "refine_skew_top", "uniqueness_f64", "cloud"};

int set_err(rsm_ctx *c, int code, const char *fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

// ---- cv::getStructuringElement(MORPH_ELLIPSE) row spans (OpenCV 2.4; see oracle + DESIGN.md) ----
void ellipse_spans(int k, std::vector<int> &j1, std::vector<int> &j2) {
    j1.assign(k, 0);
    j2.assign(k, 0);
    const int r = k / 2, c = k / 2;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    for (int i = 0; i < k; i++) {
        const int dy = i - r;
        if (abs(dy) <= r) {
            const int dx = (int)lrint(c * sqrt((r * r - dy * dy) * inv_r2));
            j1[i] = (c - dx > 0) ? c - dx : 0;
            j2[i] = (c + dx + 1 < k) ? c + dx + 1 : k;
        }
    }
}

// ------------------------------------------------------------------------------------------------
extern "C" const char *rsm_version(void) { return "rsm-mi355 0.3 (gfx950)"; }
extern "C" int rsm_abi_version(void) { return RSM_ABI_VERSION; }
extern "C" int rsm_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0;
}

extern "C" const char *rsm_last_error(const rsm_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

extern "C" int rsm_create(rsm_ctx **out, int hip_device) {
    if (!out) return RSM_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RSM_E_HIP;
    if (hip_device < 0 || hip_device >= ndev) return RSM_E_INVALID;
    rsm_ctx *c = new rsm_ctx();
    c->device = hip_device;
    {
        static std::atomic<int> g_ordinal[RSM_MAX_DEVICES];
        c->ordinal = hip_device < RSM_MAX_DEVICES ? g_ordinal[hip_device].fetch_add(1) : 0; // which share of the CUs option cu_share gives it
    }
    // (stream priorities were measured and dropped: a high-priority main stream next to low-priority sweep streams ran
    //  two pairs in flight at 164 Mdisp/s instead of 210)
    if (hipSetDevice(hip_device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_pyr, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_cloudprep, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_heavy, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_heavy2, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        delete c;
        return RSM_E_HIP;
    }
    if (const char *e = getenv("RSM_FILTER_LOW_PRIORITY")) c->opt_filter_low_priority = atoi(e) != 0; // (A/B of the adapter loop, whose contexts take no options)
    for (int k = 0; k < RSM_MAX_LEVELS; k++)
        if (hipEventCreateWithFlags(&c->ev_prep[k], hipEventDisableTiming) != hipSuccess) {
            delete c;
            return RSM_E_HIP;
        }
    *out = c;
    return RSM_OK;
}

static void free_workspace(rsm_ctx *c) {
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    for (void *p : c->allocs) (void)hipFree(p);
    c->allocs.clear();
    c->pack16 = nullptr;
    c->pack_nrm = nullptr;
    c->cap_px = 0;
    c->have_pair = c->have_result = false;
}

extern "C" void rsm_destroy(rsm_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_workspace(c);
    filter_arena_destroy(c->filt_arena);
    poisson_mesh_free(&c->pmesh);
    if (c->mcol_rgb) (void)hipFree(c->mcol_rgb);
    if (c->mcol_best) (void)hipFree(c->mcol_best);
    for (auto &e : c->evpool) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    (void)hipEventDestroy(c->ev_pyr);
    (void)hipEventDestroy(c->ev_cloudprep);
    heavy_forget(c);
    (void)hipEventDestroy(c->ev_heavy);
    (void)hipEventDestroy(c->ev_heavy2);
    (void)hipEventDestroy(c->ev_fork);
    (void)hipEventDestroy(c->ev_join);
    for (int k = 0; k < RSM_MAX_LEVELS; k++) (void)hipEventDestroy(c->ev_prep[k]);
    if (c->ev_filter) (void)hipEventDestroy(c->ev_filter);
    if (c->stream_filter) (void)hipStreamDestroy(c->stream_filter);
    (void)hipStreamDestroy(c->stream2);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

#define DALLOC(c, p, n)                         \
    do {                                        \
        int s__ = dalloc((c), &(p), (size_t)(n)); \
        if (s__ != RSM_OK) return s__;          \
    } while (0)

static int validate(rsm_ctx *c, const rsm_pair_in *in) {
    if (!c || !in) return RSM_E_INVALID;
    if (in->pyr_levels < 1 || in->pyr_levels > RSM_MAX_LEVELS) return set_err(c, RSM_E_INVALID, "pyr_levels");
    if (in->radius < 1 || in->radius > 15) return set_err(c, RSM_E_INVALID, "radius");
    // 16384: the widest margin row k_order can hold in a CU's 160 KB of LDS (6.2 B per column), and int16 columns
    if (in->width <= 0 || in->height <= 0 || in->width > 16384 || in->height > 16384)
        return set_err(c, RSM_E_INVALID, "size (1..16384)");
    const int top = 1 << (in->pyr_levels - 1);
    if ((in->width % top) || (in->height % top)) return set_err(c, RSM_E_INVALID, "size not divisible by 2^(levels-1)");
    if ((in->width / top) <= 2 * in->radius + 2 || (in->height / top) <= 2 * in->radius + 2)
        return set_err(c, RSM_E_INVALID, "lowest level smaller than the match window");
    if (!in->image[0] || !in->image[1] || !in->mask[0] || !in->mask[1]) return set_err(c, RSM_E_INVALID, "null image/mask");
    if (in->origin_width <= 0) return set_err(c, RSM_E_INVALID, "origin_width");
    return RSM_OK;
}

static int ensure_workspace(rsm_ctx *c, const rsm_pair_in *in) {
    const size_t px = (size_t)in->width * in->height;
    const bool same = c->N > 0 && c->cap_px == px && c->N == in->pyr_levels && c->Wk[c->N - 1] == in->width;
    c->in = *in;
    c->in.image[0] = c->in.image[1] = c->in.mask[0] = c->in.mask[1] = nullptr;
    if (same) return RSM_OK;
    free_workspace(c);
    const int N = in->pyr_levels;
    c->N = N;
    for (int k = N - 1; k >= 0; k--) {
        c->Wk[k] = in->width >> (N - 1 - k);
        c->Hk[k] = in->height >> (N - 1 - k);
        for (int v = 0; v < 2; v++) {
            DALLOC(c, c->img[k][v], (size_t)c->Wk[k] * c->Hk[k] * 3);
            DALLOC(c, c->msk[k][v], (size_t)c->Wk[k] * c->Hk[k]);
            DALLOC(c, c->S1[k][v], (size_t)c->Wk[k] * c->Hk[k]);
            DALLOC(c, c->S2[k][v], (size_t)c->Wk[k] * c->Hk[k]);
            DALLOC(c, c->img4[k][v], (size_t)c->Wk[k] * c->Hk[k]);
            DALLOC(c, c->d16i[k][v], (size_t)c->Wk[k] * c->Hk[k]);
            DALLOC(c, c->d16m[k][v], (size_t)c->Wk[k] * c->Hk[k]);
            DALLOC(c, c->d16s[k][v], (size_t)c->Wk[k] * c->Hk[k]);
        }
    }
    DALLOC(c, c->d_margins, RSM_MAX_LEVELS * 2 * 4);
    DALLOC(c, c->tmp1, px);
    DALLOC(c, c->tmp2, px);
    for (int v = 0; v < 2; v++) {
        DALLOC(c, c->d16a[v], px);
        if (v == 0) DALLOC(c, c->cloud_flags, px);
        DALLOC(c, c->BL[v], px);
        DALLOC(c, c->BR[v], px);
        for (int i = 0; i < 3; i++) DALLOC(c, c->f64[i][v], px);
        DALLOC(c, c->nv[v], px / 4 + 16);
        DALLOC(c, c->rf_key[v], px);     // both ways' keys of a pixel in one dword
        DALLOC(c, c->rf_ent[v], 2 * px); // a (pwp, delta) record per way
    }
    DALLOC(c, c->rf_cnt, 32 + 2 * (size_t)in->height); // level k uses rf_cnt + k: [0] wide-pixel count, [16 + dir * H + y] Rematch pixels of a row
    DALLOC(c, c->rf_list, std::max(2 * px + 64, 2 * SETB_SCRATCH(in->width)));
    DALLOC(c, c->tie_list, 2 * px + 64);
    DALLOC(c, c->wrow, NCC_WROW_INTS((size_t)in->height)); // per (direction, row) counters and the row kernels' row lists (rsm_dev.h)
    // (a shard that fills drops further records: the entries stay in the launch's LDS copy, and a later sweep that needs one misses
    // again -- costs time, never bits.  With the re-key in front of the early launches they list about as few as the settled ones.)
    c->upd_cap = (int)std::min<size_t>(65536, std::max<size_t>(1024, px / 8));
    DALLOC(c, c->upd_list, (size_t)RF_UPD_SHARDS * c->upd_cap);
    DALLOC(c, c->upd_list2, (size_t)RF_UPD_SHARDS * c->upd_cap);
    DALLOC(c, c->upd_cnt2, 2 * RF_UPD_SHARDS);
    DALLOC(c, c->upd_cnt, 2 * RF_UPD_SHARDS);
    DALLOC(c, c->tie_cnt, 2 * RSM_MAX_LEVELS);
    DALLOC(c, c->prefix, (size_t)(in->width + 1) * in->height);
    DALLOC(c, c->blk, CLOUD_BLOCKS(in->width, in->height));
    DALLOC(c, c->d_j1, 4096);
    DALLOC(c, c->d_j2, 4096);
    DALLOC(c, c->d_cj1, 4096);
    DALLOC(c, c->d_cj2, 4096);
    DALLOC(c, c->row_count, (size_t)in->height);
    DALLOC(c, c->row_offset, (size_t)in->height);
    DALLOC(c, c->d_npoints, 2);
    DALLOC(c, c->d_vtop, 2);
    DALLOC(c, c->d_q, 16);
    DALLOC(c, c->d_R, 9);
    DALLOC(c, c->d_T, 3);
    DALLOC(c, c->xyz, px * 3);
    DALLOC(c, c->bgr, px * 3);
    c->cap_px = px;
    return RSM_OK;
}

// The per-pair constants of DisparityToCloud travel with the pair: ellipse spans for ceil(0.02 * rows) (.cpp:703),
// Q with its last column scaled (.cpp:692,698), R_final, T_final.  Synchronous (the sources are temporaries).
static int upload_cloud_params(rsm_ctx *c) {
    const int k = c->N - 1, H = c->Hk[k];
    const int ksize = (int)ceil(0.02 * H);
    if (ksize > 4096) return set_err(c, RSM_E_INVALID, "erode size");
    std::vector<int> j1, j2;
    ellipse_spans(ksize, j1, j2);
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->d_cj1, j1.data(), sizeof(int) * ksize, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->d_cj2, j2.data(), sizeof(int) * ksize, hipMemcpyHostToDevice, st));
    double q[16];
    memcpy(q, c->in.Q, sizeof q);
    const double scale = (double)c->Wk[0] / c->in.origin_width * (1 << k); // .cpp:692
    for (int i = 0; i < 4; i++) q[i * 4 + 3] *= scale;                     // .cpp:698
    HIPCHK(c, hipMemcpyAsync(c->d_q, q, sizeof q, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->d_R, c->in.R_final, sizeof(double) * 9, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->d_T, c->in.T_final, sizeof(double) * 3, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return RSM_OK;
}

static int upload_common(rsm_ctx *c, const rsm_pair_in *in, hipMemcpyKind kind) {
    int s = validate(c, in);
    if (s != RSM_OK) return s;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream2)); // nothing of a previous (possibly failed) run may still be in flight
    s = ensure_workspace(c, in);
    if (s != RSM_OK) return s;
    const int top = c->N - 1;
    const size_t px = (size_t)in->width * in->height;
    for (int v = 0; v < 2; v++) {
        HIPCHK(c, hipMemcpyAsync(c->img[top][v], in->image[v], px * 3, kind, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->msk[top][v], in->mask[v], px, kind, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s = upload_cloud_params(c);
    if (s != RSM_OK) return s;
    c->have_pair = true;
    c->have_result = false;
    return RSM_OK;
}

extern "C" int rsm_upload_pair(rsm_ctx *c, const rsm_pair_in *in) { return upload_common(c, in, hipMemcpyHostToDevice); }
extern "C" int rsm_upload_pair_device(rsm_ctx *c, const rsm_pair_in *in) {
    return upload_common(c, in, hipMemcpyDeviceToDevice);
}

// ---- profiling helpers --------------------------------------------------------------------------
int prof_slot(rsm_ctx *c, int stage) { // next event pair of the pool
    if (c->ev_used == c->evpool.size()) {
        EvPair e{};
        (void)hipEventCreate(&e.a);
        (void)hipEventCreate(&e.b);
        c->evpool.push_back(e);
    }
    c->evpool[c->ev_used].stage = stage;
    return (int)c->ev_used++;
}
// A stage of rsm_run_pair on the main stream, for rsm_profile_*: event a where the bracket is made, event b where its scope
// ends, and the stage's launches and bytes booked there.
struct StageScope {
    rsm_ctx *c;
    int stage, slot = -1, launches;
    double bytes;
    StageScope(rsm_ctx *c_, int stage_, int launches_, double bytes_) : c(c_), stage(stage_), launches(launches_), bytes(bytes_) {
        if (!c->profile || !c->profile_stages) return;
        slot = prof_slot(c, stage);
        (void)hipEventRecord(c->evpool[slot].a, c->stream);
    }
    ~StageScope() {
        if (slot < 0) return;
        (void)hipEventRecord(c->evpool[slot].b, c->stream);
        c->prof_launches[stage] += launches;
        c->prof_bytes[stage] += bytes;
    }
    StageScope(const StageScope &) = delete;
    StageScope &operator=(const StageScope &) = delete;
};

// ---- options ------------------------------------------------------------------------------------
// The plain ones: a flag (value != 0) or a value clamped to [lo, hi].  Their defaults are the member initialisers (rsm_ctx.h),
// what they do is told in include/rsm.h.
enum OptKind { OPT_BOOL, OPT_CLAMP };
struct OptRow {
    const char *name;
    int rsm_ctx::*member;
    OptKind kind;
    long long lo, hi;
};
static const OptRow kOptions[] = {
    {"ncc_bytes", &rsm_ctx::opt_ncc_bytes, OPT_BOOL, 0, 0},
    {"ncc_slide_max", &rsm_ctx::opt_ncc_slide_max, OPT_CLAMP, 0, 1000000},
    {"no_exact", &rsm_ctx::opt_no_exact, OPT_BOOL, 0, 0},
    {"heavy_exclusive", &rsm_ctx::opt_heavy_exclusive, OPT_CLAMP, 0, 2},
    {"heavy_from_sweep", &rsm_ctx::opt_heavy_from_sweep, OPT_CLAMP, 1, 100000},
    {"heavy_min_px", &rsm_ctx::opt_heavy_min_px, OPT_CLAMP, 0, 2000000000},
    {"heavy_lanes", &rsm_ctx::opt_heavy_lanes, OPT_CLAMP, 1, 2},
    {"shared_gpu", &rsm_ctx::opt_shared_gpu, OPT_BOOL, 0, 0},
    {"refine_prefill", &rsm_ctx::opt_refine_prefill, OPT_BOOL, 0, 0},
    {"refine_rekey_until", &rsm_ctx::opt_refine_rekey_until, OPT_CLAMP, 0, 100000},
    {"refine_rekey_side", &rsm_ctx::opt_refine_rekey_side, OPT_BOOL, 0, 0},
    {"refine_split", &rsm_ctx::opt_refine_split, OPT_CLAMP, 0, 2}, // 2: also with pairs in flight (A/B)
    {"refine_skew_from", &rsm_ctx::opt_refine_skew_from, OPT_CLAMP, 0, 100000},
    {"refine_skew_T", &rsm_ctx::opt_refine_skew_T, OPT_CLAMP, 2, 4},
    {"refine_skew_min_px", &rsm_ctx::opt_refine_skew_min_px, OPT_CLAMP, 0, 2000000000},
    {"refine_skew_waves", &rsm_ctx::opt_refine_skew_waves, OPT_CLAMP, 1, 1000000},
    {"refine_skew_waves_alone", &rsm_ctx::opt_refine_skew_waves_alone, OPT_CLAMP, 0, 1000000},
    {"refine_skew_waves_low", &rsm_ctx::opt_refine_skew_waves_low, OPT_CLAMP, 0, 1000000},
    {"refine_skew_rows", &rsm_ctx::opt_refine_skew_rows, OPT_CLAMP, 0, 1000000},
    {"refine_skew_prio", &rsm_ctx::opt_refine_skew_prio, OPT_CLAMP, 0, 40},
    {"refine_tile_from", &rsm_ctx::opt_refine_tile_from, OPT_CLAMP, 1, 100000},
    {"refine_tile_min_px", &rsm_ctx::opt_refine_tile_min_px, OPT_CLAMP, 0, 2000000000},
    {"refine_upd_cap", &rsm_ctx::opt_refine_upd_cap, OPT_CLAMP, 0, 1LL << 30},
    {"filter_wg_max", &rsm_ctx::opt_filter_wg_max, OPT_CLAMP, 0, 1LL << 30},
    {"filter_normals_window", &rsm_ctx::opt_filter_normals_window, OPT_CLAMP, 0, 40},
    {"filter_low_priority", &rsm_ctx::opt_filter_low_priority, OPT_BOOL, 0, 0},
    {"filter_list", &rsm_ctx::opt_filter_list, OPT_CLAMP, 0, 31}, // bit 0: the 24-pixel list pass, bit 1: the 40-pixel one, bit 2: the wave passes (80, 160, ... pixels) for what they leave, bits 3 / 4: the 24- / 40-pixel pass in the wave form too
    {"filter_window", &rsm_ctx::opt_filter_window, OPT_CLAMP, 0, 24}, // 0 off, 1 default, else the radius
};

// The options that do more than that.
static int set_no_rowgemm(rsm_ctx *c, long long value) {
    c->opt_no_rowgemm = value != 0 ? 1 : 0;
    return RSM_OK;
}
static int set_wide_rows(rsm_ctx *c, long long value) {
    c->opt_no_rowgemm = (value >= 0 && value <= 3) ? (int)value : 0;
    return RSM_OK;
}
static int set_ncc_mid(rsm_ctx *c, long long value) {
    c->opt_ncc_mid = value <= 0 ? 0 : (int)std::max(8LL, std::min(value, 160LL));
    return RSM_OK;
}
static int set_meshcolor_big_box(rsm_ctx *c, long long value) { // (a 64-bit member)
    c->opt_meshcolor_big_box = std::max(1LL, std::min(value, 1LL << 20));
    return RSM_OK;
}
static int set_refine_skew_uw(rsm_ctx *c, long long value) { // an even number of columns (the state row's 16-byte pieces start on even columns)
    if (value < 0 || value > 62 || (value & 1)) return set_err(c, RSM_E_INVALID, "refine_skew_uw %lld: 0 (= 66 - 2T) or an even number <= 66 - 2T", value);
    c->opt_refine_skew_uw = (int)value;
    return RSM_OK;
}
static int set_refine_tile_T(rsm_ctx *c, long long value) {
    if (value != 0 && (value < 2 || value > RF_TILE_MAXT)) return set_err(c, RSM_E_INVALID, "refine_tile_T %lld: 0 (off) or 2 .. %d", value, RF_TILE_MAXT);
    c->opt_refine_tile_T = (int)value;
    return RSM_OK;
}
static int set_filter_ladder_h(rsm_ctx *c, long long value) { // the bit pattern of a positive finite float32: the first ladder level's search radius; 0: from the sample
    if (value < 0 || value >= 0x7f800000LL) return set_err(c, RSM_E_INVALID, "filter_ladder_h %lld: 0 or the bit pattern of a positive finite float", value);
    uint32_t bits = (uint32_t)value;
    memcpy(&c->filt_route.h0, &bits, sizeof bits);
    return RSM_OK;
}
// Contexts that share a GPU each on their own share of the compute units (the `ordinal % n`-th of n equal ranges of the
// CU mask, hipExtStreamCreateWithCUMask) instead of all of them on the whole chip; 0 / 1 = the whole chip.
static int set_cu_share(rsm_ctx *c, long long value) {
    const int n = (int)std::max(0LL, std::min(value, 64LL));
    if (c->in_run.load()) return set_err(c, RSM_E_STATE, "cu_share: the context is inside rsm_run_pair (its streams are in use)");
    if (hipSetDevice(c->device) != hipSuccess) return set_err(c, RSM_E_HIP, "hipSetDevice");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) return set_err(c, RSM_E_HIP, "hipGetDeviceProperties");
    const int ncu = prop.multiProcessorCount;
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->stream2);
    hipStream_t s1 = nullptr, s2 = nullptr;
    hipError_t e1, e2;
    if (n > 1) {
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
        const int idx = c->ordinal % n, lo = (int)((long long)idx * ncu / n), hi = (int)((long long)(idx + 1) * ncu / n);
        for (int i = lo; i < hi; i++) mask[(size_t)i / 32] |= 1u << (i & 31);
        e1 = hipExtStreamCreateWithCUMask(&s1, (uint32_t)mask.size(), mask.data());
        e2 = hipExtStreamCreateWithCUMask(&s2, (uint32_t)mask.size(), mask.data());
    } else {
        e1 = hipStreamCreateWithFlags(&s1, hipStreamNonBlocking);
        e2 = hipStreamCreateWithFlags(&s2, hipStreamNonBlocking);
    }
    if (e1 != hipSuccess || e2 != hipSuccess) {
        if (s1) (void)hipStreamDestroy(s1);
        if (s2) (void)hipStreamDestroy(s2);
        return set_err(c, RSM_E_HIP, "cu_share: stream creation failed");
    }
    (void)hipStreamDestroy(c->stream);
    (void)hipStreamDestroy(c->stream2);
    c->stream = s1;
    c->stream2 = s2;
    c->opt_cu_share = n;
    return RSM_OK;
}
static const struct {
    const char *name;
    int (*set)(rsm_ctx *c, long long value);
} kSpecialOptions[] = {
    {"no_rowgemm", set_no_rowgemm},
    {"wide_rows", set_wide_rows},
    {"ncc_mid", set_ncc_mid},
    {"meshcolor_big_box", set_meshcolor_big_box},
    {"refine_skew_uw", set_refine_skew_uw},
    {"refine_tile_T", set_refine_tile_T},
    {"filter_ladder_h", set_filter_ladder_h},
    {"cu_share", set_cu_share},
};

extern "C" int rsm_set_option(rsm_ctx *c, const char *name, long long value) {
    if (!c || !name) return RSM_E_INVALID;
    if (!strncmp(name, "filter_", 7)) c->filt_memo_radius = 0; // (the cloud filter's own options: it probes its window radius afresh)
    for (const OptRow &o : kOptions)
        if (!strcmp(name, o.name)) {
            c->*o.member = o.kind == OPT_BOOL ? (int)(value != 0) : (int)std::max(o.lo, std::min(value, o.hi));
            return RSM_OK;
        }
    for (const auto &o : kSpecialOptions)
        if (!strcmp(name, o.name)) return o.set(c, value);
    return set_err(c, RSM_E_INVALID, "unknown option %s", name);
}

extern "C" int rsm_profile_enable(rsm_ctx *c, int on) {
    if (!c) return RSM_E_INVALID;
    c->profile = on != 0;
    c->profile_stages = on == 1; // 2: only the dominant kernel's launches are bracketed
    for (int i = 0; i < ST_COUNT; i++) { // the counters accumulate over the runs that follow
        c->prof_ms[i] = 0;
        c->prof_launches[i] = 0;
        c->prof_bytes[i] = 0;
    }
    return RSM_OK;
}
extern "C" int rsm_profile_stage_count(void) { return ST_COUNT; }
extern "C" const char *rsm_profile_stage_name(int s) { return (s >= 0 && s < ST_COUNT) ? kStageNames[s] : ""; }
extern "C" int rsm_profile_get(rsm_ctx *c, double *ms, int64_t *launches, double *bytes) {
    if (!c) return RSM_E_INVALID;
    for (int i = 0; i < ST_COUNT; i++) {
        if (ms) ms[i] = c->prof_ms[i];
        if (launches) launches[i] = c->prof_launches[i];
        if (bytes) bytes[i] = c->prof_bytes[i];
    }
    return RSM_OK;
}

// ---- stage-argument assembly ---------------------------------------------------------------------
static StageArgs level_args(rsm_ctx *c, int k) {
    StageArgs a{};
    a.ndir = 2;
    a.W = c->Wk[k];
    a.H = c->Hk[k];
    a.Wp = k > 0 ? c->Wk[k - 1] : 0;
    a.Hp = k > 0 ? c->Hk[k - 1] : 0;
    a.r = c->in.radius;
    a.offset = c->in.offset;
    a.ws = c->in.ws;
    a.rf_list = c->rf_list;
    a.ncc_cnt = c->rf_cnt + k; // a counter per level, zeroed together at the start of the run
    a.tie_list = c->tie_list;
    a.tie_cnt = c->tie_cnt + 2 * k;
    a.wrow = c->wrow;
    a.opt_no_rowgemm = c->opt_no_rowgemm;
    a.ncc_mid = c->opt_ncc_mid;
    a.ncc_slide_max = c->opt_ncc_slide_max;
    a.upd_list = c->upd_list;
    a.upd_cnt = c->upd_cnt;
    a.upd_cap = c->upd_cap;
    a.rf_stride = c->cap_px;
    a.opt_ncc_bytes = c->opt_ncc_bytes;
    a.opt_no_exact = c->opt_no_exact;
    for (int v = 0; v < 2; v++) {
        DirArgs &d = a.d[v];
        const int o = 1 - v;
        d.img_own = c->img[k][v];
        d.img_oth = c->img[k][o];
        d.img4_own = c->img4[k][v];
        d.img4_oth = c->img4[k][o];
        d.mask_own = c->msk[k][v];
        d.mask_oth = c->msk[k][o];
        d.S1_own = c->S1[k][v];
        d.S2_own = c->S2[k][v];
        d.S1_oth = c->S1[k][o];
        d.S2_oth = c->S2[k][o];
        d.own = c->mg[k][v];
        d.oth = c->mg[k][o];
        d.BL = c->BL[v];
        d.BR = c->BR[v];
        d.parent_nv = c->nv[v];
        d.rf_key = c->rf_key[v];
        d.rf_ent = c->rf_ent[v];
    }
    return a;
}


// ---- rsm_run_pair's steps, in the order they run --------------------------------------------------

// ConstructPyrm, .cpp:1040-1053 (top level = uploaded images).  The main stream needs the masks (margins) first;
// everything that depends on the images or the top mask only goes to the side stream and is made while the small
// levels (launch-latency bound, the GPU mostly idle) are matched: the image pyramid, every level's BGRX copy and
// NCC window sums (level k waits for ev_prep[k]), and the cloud's bad-pixel prefix + block map (ev_cloudprep).
static int prepare_side_stream(rsm_ctx *c) {
    const int N = c->N, r = c->in.radius;
    hipStream_t s2 = c->stream2;
    HIPCHK(c, hipEventRecord(c->ev_pyr, c->stream)); // everything enqueued before this run
    HIPCHK(c, hipStreamWaitEvent(s2, c->ev_pyr, 0));
    for (int k = N - 2; k >= 0; k--)
        for (int v = 0; v < 2; v++) launch_pyr_down(c->img[k + 1][v], c->Wk[k + 1], c->Hk[k + 1], 3, c->img[k][v], s2);
    for (int k = 0; k < N; k++) {
        const int W = c->Wk[k], H = c->Hk[k];
        for (int v = 0; v < 2; v++) {
            launch_bgr_to_bgrx(c->img[k][v], W, H, c->img4[k][v], s2);
            launch_box_sums(c->img4[k][v], W, H, r, c->tmp1, c->tmp2, c->S1[k][v], c->S2[k][v], s2);
            // the maps the initial match and the median filter write into start as NOMATCH everywhere (.cpp:772)
            launch_fill_i16(c->d16i[k][v], (size_t)W * H, (int16_t)NOMATCH, s2);
            launch_fill_i16(c->d16m[k][v], (size_t)W * H, (int16_t)NOMATCH, s2);
            launch_fill_i16(c->d16s[k][v], (size_t)W * H, (int16_t)NOMATCH, s2);
        }
        HIPCHK(c, hipEventRecord(c->ev_prep[k], s2));
    }
    launch_bad_prefix(c->msk[N - 1][0], c->Wk[N - 1], c->Hk[N - 1], c->prefix, s2);
    launch_bad_blocks(c->prefix, c->Wk[N - 1], c->Hk[N - 1], c->blk, s2);
    HIPCHK(c, hipEventRecord(c->ev_cloudprep, s2));
    return RSM_OK;
}

// The mask pyramid and FindMargin for every level and view (.cpp:51-52: they depend on the masks only), down to the host.
// Rematch -> SetBoundary_smooth exits on a degenerate margin (.cpp:827-830): every level's margin is known here, so that
// is decided before any level is enqueued, and no side-stream work is left behind that the next call could collide with.
static int find_margins(rsm_ctx *c) {
    const int N = c->N;
    hipStream_t st = c->stream;
    {
        StageScope ps(c, ST_PYRAMID, 2 * (N - 1), 14.0 * (double)c->Wk[N - 1] * c->Hk[N - 1]);
        for (int k = N - 2; k >= 0; k--)
            for (int v = 0; v < 2; v++) launch_pyr_down(c->msk[k + 1][v], c->Wk[k + 1], c->Hk[k + 1], 1, c->msk[k][v], st);
    }
    {
        StageScope ps(c, ST_MARGIN, 1, 0);
        const uint8_t *masks[RSM_MAX_LEVELS * 2];
        int Ws[RSM_MAX_LEVELS * 2], Hs[RSM_MAX_LEVELS * 2];
        for (int k = 0; k < N; k++)
            for (int v = 0; v < 2; v++) {
                masks[k * 2 + v] = c->msk[k][v];
                Ws[k * 2 + v] = c->Wk[k];
                Hs[k * 2 + v] = c->Hk[k];
            }
        launch_find_margin_batch(2 * N, masks, Ws, Hs, c->in.radius, c->d_margins, c->h_margin_init, st);
        HIPCHK(c, hipMemsetAsync(c->rf_cnt, 0, sizeof(int) * 16, st)); // the levels' wide-pixel counters
        HIPCHK(c, hipMemsetAsync(c->tie_cnt, 0, sizeof(int) * 2 * RSM_MAX_LEVELS, st));
    }
    int hm[RSM_MAX_LEVELS * 2 * 4];
    HIPCHK(c, hipMemcpyAsync(hm, c->d_margins, sizeof(int) * N * 2 * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int k = 0; k < N; k++)
        for (int v = 0; v < 2; v++) {
            const int *m = hm + (k * 2 + v) * 4;
            c->mg[k][v] = Mg{m[2], m[3], m[0], m[1]};
        }
    for (int k = 0; k < N; k++)
        if (degenerate(c->mg[k][0]) || degenerate(c->mg[k][1])) {
            (void)hipStreamSynchronize(c->stream2);
            return set_err(c, RSM_E_DEGENERATE_MARGIN, "level %d: YL>=YR || XL>=XR", k);
        }
    launch_count_masked(c->msk[N - 1][0], c->Wk[N - 1], c->Hk[N - 1], c->mg[N - 1][0], c->d_vtop, st);
    return RSM_OK;
}

// UniquenessContraint (.cpp:75, :86, :109): own against other, other against own, own again
template <typename F, typename P>
static void uniq3(F launcher, P *p0, P *p1, int W, int H, const Mg &m0, const Mg &m1, hipStream_t st) {
    launcher(p0, p1, W, H, m0, m1, st);
    launcher(p1, p0, W, H, m1, m0, st);
    launcher(p0, p1, W, H, m0, m1, st);
}

// DisparityRefine (.cpp:95-98): int16 d16m[k] -> fp64, 30 + 30k Jacobi sweeps, and UniquenessContraint<double> (.cpp:109) on
// the refined maps.  f64[par] holds the previous level's disparity; returns the buffer that holds this level's.
static int refine_level(rsm_ctx *c, StageArgs &a, int k, int par, double Pk) {
    hipStream_t st = c->stream;
    const bool top = k == c->N - 1;
    const int iters = 30 + k * 30;
    const int ia = (par + 1) % 3, ib = (par + 2) % 3;
    {
        StageScope ps(c, ST_REFINE_INIT, 1, 12.0 * Pk);
        for (int v = 0; v < 2; v++) {
            a.d[v].d16_in = c->d16m[k][v];
            a.d[v].f64_a = c->f64[ia][v];
            a.d[v].f64_b = c->f64[ib][v];
        }
        launch_refine_init(a, st);
    }
    bool inB = false;
    {
        StageScope ps(c, top ? ST_REFINE_SWEEP_TOP : ST_REFINE_SWEEP, 0, 32.0 * Pk * iters);
        a.flag = top;
        double *bufA[2] = {c->f64[ia][0], c->f64[ia][1]}, *bufB[2] = {c->f64[ib][0], c->f64[ib][1]};
        ps.launches = refine_sweeps(c, a, bufA, bufB, iters, st, top, &inB, Pk);
    }
    const int cur = inB ? ib : ia;
    StageScope ps(c, ST_UNIQ64, 3, 72.0 * Pk);
    uniq3(launch_uniq_f64, c->f64[cur][0], c->f64[cur][1], a.W, a.H, c->mg[k][0], c->mg[k][1], st);
    return cur;
}

// MatchOneLayer (.cpp:36-113) for level k, stage order kept exactly.  `par` is the fp64 buffer holding the previous level's
// disparity (this is `disparity[]`); returns the buffer holding this level's, or a negative status.
static int match_level(rsm_ctx *c, int k, int par) {
    hipStream_t st = c->stream;
    const int W = c->Wk[k], H = c->Hk[k];
    StageArgs a = level_args(c, k);
    const Extent e0 = margin_extent(a.d[0].own), e1 = margin_extent(a.d[1].own);
    const double Pk = 0.5 * ((double)e0.cols * e0.rows + (double)e1.cols * e1.rows); // pixels of a margin, the two views averaged
    auto maps = [&](int16_t *const in[2], int16_t *const out[2]) {
        for (int v = 0; v < 2; v++) {
            a.d[v].d16_in = in[v];
            a.d[v].d16_out = out[v];
        }
    };
    int16_t **d16i = c->d16i[k], **d16s = c->d16s[k], **d16m = c->d16m[k];
    { // what the main stream still has to wait for
        StageScope ps(c, ST_BOXSUM, 6, 0);
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_prep[k], 0));
    }
    { // initial match (.cpp:53-62) -> d16i[k] (NOMATCH-filled by the side stream)
        StageScope ps(c, ST_INITIAL_MATCH, k == 0 ? 3 : 6, 24.0 * Pk);
        maps(d16i, d16i);
        HIPCHK(c, hipMemsetAsync(c->wrow, 0, sizeof(int32_t) * 2 * (size_t)H, st)); // wide pixels per row of this level
        if (k == 0) {
            launch_ncc_argmax(a, 0, st);
        } else {
            for (int v = 0; v < 2; v++) a.d[v].parent = c->f64[par][v];
            launch_next_valid2(c->f64[par][0], c->f64[par][1], a.Wp, a.Hp, c->nv[0], c->nv[1], st);
            launch_hl_interval(a, st);
            launch_ncc_argmax(a, 1, st);
        }
    }
    { // SmoothConstraint (.cpp:66-67): d16i[k] -> d16s[k] (both NOMATCH outside the margins: no copy)
        StageScope ps(c, ST_SMOOTH, 1, 8.0 * Pk);
        maps(d16i, d16s);
        launch_smooth(a, st, false);
    }
    { // OrderConstraint (.cpp:71-72): d16s[k] in place
        StageScope ps(c, ST_ORDER, 1, 8.0 * Pk);
        maps(d16s, d16s);
        const hipError_t oe = launch_order(a, st);
        if (oe != hipSuccess) {
            (void)hipStreamSynchronize(c->stream2);
            (void)hipStreamSynchronize(st);
            return set_err(c, RSM_E_HIP, "level %d: OrderConstraint's margin rows do not fit the LDS: %s", k, hipGetErrorString(oe));
        }
    }
    { // UniquenessContraint<short> (.cpp:75)
        StageScope ps(c, ST_UNIQ16, 3, 18.0 * Pk);
        uniq3(launch_uniq_s16, d16s[0], d16s[1], W, H, c->mg[k][0], c->mg[k][1], st);
    }
    { // Rematch (.cpp:80-81): SetBoundary_smooth + NCC on still-unmatched pixels, in place
        StageScope ps(c, ST_REMATCH, 3, 46.0 * Pk);
        launch_set_boundary(a, st, true);
        launch_ncc_argmax(a, 2, st);
    }
    { // UniquenessContraint<short> (.cpp:86)
        StageScope ps(c, ST_UNIQ16, 3, 18.0 * Pk);
        uniq3(launch_uniq_s16, d16s[0], d16s[1], W, H, c->mg[k][0], c->mg[k][1], st);
    }
    { // MedianFilter (.cpp:89-90): d16s[k] -> d16m[k] (pre-filled NOMATCH, .cpp:772)
        StageScope ps(c, ST_MEDIAN, 3, 10.0 * Pk);
        maps(d16s, d16m);
        launch_median(a, st);
    }
    const int cur = refine_level(c, a, k, par, Pk);
    // a launch that could not start (e.g. an LDS request the input drove too high) must not go unnoticed
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        (void)hipStreamSynchronize(c->stream2);
        (void)hipStreamSynchronize(st);
        return set_err(c, RSM_E_HIP, "level %d: kernel launch failed: %s", k, hipGetErrorString(le));
    }
    return cur;
}

// DisparityToCloud<double>(disparity[0], maskPyrm[top][0], Q, top, true) (.cpp:29) from f64[par], and the run's results
static int make_cloud(rsm_ctx *c, int par) {
    hipStream_t st = c->stream;
    const int k = c->N - 1, W = c->Wk[k], H = c->Hk[k];
    {
        const Mg &m = c->mg[k][0];
        StageScope ps(c, ST_CLOUD, 4, 28.0 * (double)(m.XR - m.XL + 1) * (m.YR - m.YL + 1));
        const int ksize = (int)ceil(0.02 * H); // .cpp:703; spans, Q, R, T: upload_cloud_params
        HIPCHK(c, hipStreamWaitEvent(st, c->ev_cloudprep, 0));
        launch_cloud(c->f64[par][0], c->prefix, c->img[k][0], W, H, ksize, c->d_cj1, c->d_cj2, c->d_q, c->d_R, c->d_T, m,
                     c->cloud_flags, c->blk, c->row_count, c->row_offset, c->d_npoints, c->xyz, c->bgr, (int64_t)c->cap_px, st);
    }
    int64_t np = 0;
    unsigned long long vt = 0;
    HIPCHK(c, hipMemcpyAsync(&np, c->d_npoints, sizeof np, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&vt, c->d_vtop, sizeof vt, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipGetLastError());
    c->n_points = np;
    c->v_top = (int64_t)vt;
    c->res_disp[0] = c->f64[par][0];
    c->res_disp[1] = c->f64[par][1];
    c->have_result = true;
    return RSM_OK;
}

static void collect_profile(rsm_ctx *c) { // (the run has been waited for)
    if (!c->profile) return;
    for (size_t i = 0; i < c->ev_used; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->evpool[i].a, c->evpool[i].b) == hipSuccess) c->prof_ms[c->evpool[i].stage] += ms;
    }
}

extern "C" int rsm_run_pair(rsm_ctx *c) {
    if (!c) return RSM_E_INVALID;
    if (!c->have_pair) return set_err(c, RSM_E_STATE, "rsm_run_pair before rsm_upload_pair");
    HIPCHK(c, hipSetDevice(c->device));
    RunningGuard running(c->device, &c->in_run);
    c->have_result = false;
    c->ev_used = 0;
    int s = prepare_side_stream(c);
    if (s == RSM_OK) s = find_margins(c);
    if (s != RSM_OK) return s;
    int par = 0;
    for (int k = 0; k < c->N; k++) {
        par = match_level(c, k, par);
        if (par < 0) return par;
    }
    s = make_cloud(c, par);
    if (s != RSM_OK) return s;
    collect_profile(c);
    return RSM_OK;
}

extern "C" int rsm_download_pair(rsm_ctx *c, rsm_pair_out *out) {
    if (!c || !out) return RSM_E_INVALID;
    if (!c->have_result) return set_err(c, RSM_E_STATE, "no result to download");
    HIPCHK(c, hipSetDevice(c->device));
    const int k = c->N - 1;
    const size_t px = (size_t)c->Wk[k] * c->Hk[k];
    for (int v = 0; v < 2; v++) {
        out->margin[v] = to_boundary(c->mg[k][v]); // .cpp:27-28
        if (out->disparity[v])
            HIPCHK(c, hipMemcpyAsync(out->disparity[v], c->res_disp[v], px * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    out->n_points = c->n_points;
    out->v_top = c->v_top;
    int64_t n = c->n_points;
    if (n > out->max_points) n = out->max_points;
    if (n > (int64_t)c->cap_px) n = (int64_t)c->cap_px;
    if (n > 0 && out->xyz) HIPCHK(c, hipMemcpyAsync(out->xyz, c->xyz, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n > 0 && out->bgr) HIPCHK(c, hipMemcpyAsync(out->bgr, c->bgr, (size_t)n * 3, hipMemcpyDeviceToHost, c->stream));
    if (n > 0 && out->points16) { // InsertPoint's float cast + the colour packed on the GPU: 16 instead of 27 bytes per point cross PCIe
        if (!c->pack16) {
            const int s = dalloc(c, &c->pack16, c->cap_px);
            if (s != RSM_OK) return s;
        }
        launch_pack_cloud16(c->xyz, c->bgr, n, c->pack16, c->stream);
        HIPCHK(c, hipMemcpyAsync(out->points16, c->pack16, (size_t)n * sizeof(rsm_point16), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RSM_OK;
}

// Page-locked host memory for the buffers that cross the boundary.  The reference's pipeline keeps its images and results
// in pageable cv::Mat memory (CManageData.cpp:75-78, CStereoMatching.cpp:682-761); a download into such memory goes through
// the runtime's staging copy at ~10 GB/s (34 ms for a C2 pair's two fp64 maps and cloud), into page-locked memory it is one
// DMA at the link's rate.  A cv::Mat can wrap memory from rsm_host_alloc (its user-data constructor), or memory the
// caller already owns can be page-locked in place (rsm_host_register).
extern "C" void *rsm_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) return nullptr; // (every GPU of the node may DMA into it)
    return p;
}
extern "C" void rsm_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}
extern "C" int rsm_host_register(void *p, size_t bytes) {
    if (!p || bytes == 0) return RSM_E_INVALID;
    return hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess ? RSM_OK : RSM_E_HIP;
}
extern "C" int rsm_host_unregister(void *p) {
    if (!p) return RSM_E_INVALID;
    return hipHostUnregister(p) == hipSuccess ? RSM_OK : RSM_E_HIP;
}

extern "C" int rsm_result_device(rsm_ctx *c, const double **d0, const double **d1, int64_t *n_points,
                                 const double **xyz, const uint8_t **bgr) {
    if (!c) return RSM_E_INVALID;
    if (!c->have_result) return set_err(c, RSM_E_STATE, "no result");
    if (d0) *d0 = c->res_disp[0];
    if (d1) *d1 = c->res_disp[1];
    if (n_points) *n_points = c->n_points;
    if (xyz) *xyz = c->xyz;
    if (bgr) *bgr = c->bgr;
    return RSM_OK;
}

extern "C" int rsm_export_cloud_device(rsm_ctx *c, double *d_xyz, uint8_t *d_bgr, int64_t max_points) {
    if (!c) return RSM_E_INVALID;
    if (!c->have_result) return set_err(c, RSM_E_STATE, "no result");
    HIPCHK(c, hipSetDevice(c->device));
    int64_t n = c->n_points < max_points ? c->n_points : max_points;
    if (n > (int64_t)c->cap_px) n = (int64_t)c->cap_px;
    if (n > 0 && d_xyz) HIPCHK(c, hipMemcpyAsync(d_xyz, c->xyz, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (n > 0 && d_bgr) HIPCHK(c, hipMemcpyAsync(d_bgr, c->bgr, (size_t)n * 3, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RSM_OK;
}

extern "C" int rsm_pack_cloud16(rsm_ctx *c, rsm_point16 *d_dst, int64_t max_points, int64_t *n_points) {
    if (!c) return RSM_E_INVALID;
    if (!c->have_result) return set_err(c, RSM_E_STATE, "no result");
    HIPCHK(c, hipSetDevice(c->device));
    int64_t n = c->n_points < max_points ? c->n_points : max_points;
    if (n > (int64_t)c->cap_px) n = (int64_t)c->cap_px;
    if (n > 0 && !d_dst) return RSM_E_INVALID;
    launch_pack_cloud16(c->xyz, c->bgr, n, d_dst, c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_points) *n_points = n > 0 ? n : 0;
    return RSM_OK;
}

extern "C" int rsm_match_pair(rsm_ctx *c, const rsm_pair_in *in, rsm_pair_out *out) {
    int s = rsm_upload_pair(c, in);
    if (s != RSM_OK) return s;
    s = rsm_run_pair(c);
    if (s != RSM_OK) return s;
    return rsm_download_pair(c, out);
}


// =================================================================================================
// Several pairs at once: the pair loop of CStereoMatching::MatchAllLayer (.cpp:17-33) has no cross-pair data flow,
// so pairs can be in flight together -- on one GPU (a pair's launch-latency-bound small levels and host syncs hide
// under another pair's top-level sweeps) and across the GPUs of a node (contexts on different devices).
// One host thread per context; every context keeps its own streams and workspace.
// =================================================================================================
extern "C" int rsm_run_pairs(rsm_ctx *const *ctxs, int n) { return rsm_run_pairs_repeat(ctxs, n, 1); }

extern "C" int rsm_run_pairs_repeat(rsm_ctx *const *ctxs, int n, int repeats) {
    if (!ctxs || n <= 0 || repeats < 1) return RSM_E_INVALID;
    for (int i = 0; i < n; i++) {
        if (!ctxs[i]) return RSM_E_INVALID;
        for (int j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return RSM_E_INVALID; // a context is not re-entrant
    }
    for (int i = 0; i < n; i++) { // contexts that share a device with another one of the pool: pairs in flight, never the lone-pair split
        bool shared = false;
        for (int j = 0; j < n; j++) shared |= j != i && ctxs[j]->device == ctxs[i]->device;
        ctxs[i]->pool_shared = shared;
    }
    std::vector<int> st((size_t)n, RSM_OK);
    auto loop = [&](int i) { // every context runs its resident pair `repeats` times, free of the others
        for (int k = 0; k < repeats && st[(size_t)i] == RSM_OK; k++) st[(size_t)i] = rsm_run_pair(ctxs[i]);
    };
    std::vector<std::thread> th;
    th.reserve((size_t)n - 1);
    for (int i = 1; i < n; i++) th.emplace_back(loop, i);
    loop(0);
    for (auto &t : th) t.join();
    for (int i = 0; i < n; i++) ctxs[i]->pool_shared = 0;
    for (int i = 0; i < n; i++)
        if (st[(size_t)i] != RSM_OK) return st[(size_t)i];
    return RSM_OK;
}

extern "C" int rsm_match_pairs(rsm_ctx *const *ctxs, int n_ctx, const rsm_pair_in *in, rsm_pair_out *out, int n_pairs,
                               int *status) {
    if (!ctxs || n_ctx <= 0 || n_pairs < 0 || (n_pairs > 0 && (!in || !out))) return RSM_E_INVALID;
    for (int i = 0; i < n_ctx; i++) {
        if (!ctxs[i]) return RSM_E_INVALID;
        for (int j = 0; j < i; j++)
            if (ctxs[j] == ctxs[i]) return RSM_E_INVALID;
    }
    for (int i = 0; i < n_ctx; i++) { // (see rsm_run_pairs_repeat)
        bool shared = false;
        for (int j = 0; j < n_ctx; j++) shared |= j != i && ctxs[j]->device == ctxs[i]->device;
        ctxs[i]->pool_shared = shared;
    }
    std::atomic<int> next(0);
    std::vector<int> st((size_t)n_pairs, RSM_OK);
    // Work queue: a context takes the next pair when it is free, so that upload / download of one pair (PCIe)
    // overlaps another pair's kernels and uneven pairs balance themselves.  A failed pair (e.g.
    // RSM_E_DEGENERATE_MARGIN, the reference's exit(0)) does not stop the others.
    auto worker = [&](rsm_ctx *c) {
        for (int p = next.fetch_add(1); p < n_pairs; p = next.fetch_add(1)) st[(size_t)p] = rsm_match_pair(c, &in[p], &out[p]);
    };
    const int nt = std::min(n_ctx, std::max(n_pairs, 1));
    std::vector<std::thread> th;
    for (int i = 1; i < nt; i++) th.emplace_back(worker, ctxs[i]);
    worker(ctxs[0]);
    for (auto &t : th) t.join();
    for (int i = 0; i < n_ctx; i++) ctxs[i]->pool_shared = 0;
    int first = RSM_OK;
    for (int p = 0; p < n_pairs; p++) {
        if (status) status[p] = st[(size_t)p];
        if (first == RSM_OK && st[(size_t)p] != RSM_OK) first = st[(size_t)p];
    }
    return first;
}

extern "C" int rsm_match_pairs_multi_gpu(const rsm_pair_in *in, int n_pairs, int n_gpus, int pairs_in_flight,
                                         rsm_pair_out *out, int *status) {
    if (n_pairs < 0 || (n_pairs > 0 && (!in || !out)) || n_gpus < 0 || pairs_in_flight < 0) return RSM_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RSM_E_HIP;
    if (n_gpus == 0 || n_gpus > ndev) n_gpus = ndev;
    if (pairs_in_flight == 0) pairs_in_flight = 2;
    std::vector<rsm_ctx *> ctxs;
    int s = RSM_OK;
    // context i lives on GPU i % n_gpus: the queue hands consecutive pairs to different GPUs first
    for (int i = 0; i < n_gpus * pairs_in_flight && i < std::max(n_pairs, 1) && s == RSM_OK; i++) {
        rsm_ctx *c = nullptr;
        s = rsm_create(&c, i % n_gpus);
        if (s == RSM_OK) ctxs.push_back(c);
    }
    if (s == RSM_OK) s = rsm_match_pairs(ctxs.data(), (int)ctxs.size(), in, out, n_pairs, status);
    for (rsm_ctx *c : ctxs) rsm_destroy(c);
    return s;
}

// =================================================================================================
// Rectify (CStereoMatching.cpp:117-168): host fp64 plan + device maps / remap / grey erosion.
// =================================================================================================
extern "C" int rsm_stereo_rectify(const double *K1, const double *K2, int nx, int ny, const double *R, const double *T,
                                  double *R1, double *R2, double *P1, double *P2, double *Q) {
    if (!K1 || !K2 || !R || !T || !R1 || !R2 || !P1 || !P2 || !Q || nx <= 0 || ny <= 0) return RSM_E_INVALID;
    stereo_rectify_host(K1, K2, nx, ny, R, T, R1, R2, P1, P2, Q);
    return RSM_OK;
}

extern "C" int rsm_rectify_pair(rsm_ctx *c, const rsm_rectify_in *in, int radius, double ws, int offset, int verbose,
                                rsm_rectify_out *out) {
    if (!c || !in || !out) return RSM_E_INVALID;
    if (in->origin_width <= 0 || in->origin_height <= 0 || in->lowest_width <= 0 || in->lowest_height <= 0 ||
        in->pyr_levels < 1 || in->pyr_levels > RSM_MAX_LEVELS)
        return set_err(c, RSM_E_INVALID, "rectify: sizes");
    for (int v = 0; v < 2; v++)
        if (!in->image[v] || !in->mask[v]) return set_err(c, RSM_E_INVALID, "read image error"); // .cpp:147-151
    HIPCHK(c, hipSetDevice(c->device));
    RectifyPlan plan;
    rectify_plan(in->K[0], in->K[1], in->E[0], in->E[1], in->origin_width, in->origin_height, in->lowest_width,
                 in->lowest_height, in->pyr_levels, &plan);
    rsm_pair_in pin{};
    pin.width = plan.W;
    pin.height = plan.H;
    pin.pyr_levels = in->pyr_levels;
    pin.radius = radius;
    pin.ws = ws;
    pin.offset = offset;
    pin.origin_width = in->origin_width;
    pin.verbose = verbose;
    memcpy(pin.Q, plan.Q, sizeof pin.Q);
    memcpy(pin.R_final, plan.R_final, sizeof pin.R_final);
    memcpy(pin.T_final, plan.T_final, sizeof pin.T_final);
    for (int v = 0; v < 2; v++) { // only to satisfy validate(); the rectified images are produced on the device
        pin.image[v] = in->image[v];
        pin.mask[v] = in->mask[v];
    }
    int s = validate(c, &pin);
    if (s != RSM_OK) return s;
    HIPCHK(c, hipStreamSynchronize(c->stream2)); // the maps below reuse the side stream's scratch (tmp1 / tmp2)
    s = ensure_workspace(c, &pin);
    if (s != RSM_OK) return s;
    hipStream_t st = c->stream;
    const int top = c->N - 1, W = plan.W, H = plan.H;
    const size_t opx = (size_t)in->origin_width * in->origin_height, px = (size_t)W * H;
    Tmp t(c);
    uint8_t *raw_img = t.alloc<uint8_t>(opx * 3), *raw_msk = t.alloc<uint8_t>(opx);
    if (!t.ok) return set_err(c, RSM_E_NOMEM, "rectify: raw buffers");
    std::vector<int> j1, j2;
    if (plan.ksize > 4096) return set_err(c, RSM_E_INVALID, "erode size");
    ellipse_spans(plan.ksize, j1, j2);
    HIPCHK(c, hipMemcpyAsync(c->d_j1, j1.data(), sizeof(int) * plan.ksize, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->d_j2, j2.data(), sizeof(int) * plan.ksize, hipMemcpyHostToDevice, st));
    int16_t *map1 = (int16_t *)c->tmp1;   // 4 B / pixel
    uint16_t *map2 = (uint16_t *)c->tmp2; // 2 B / pixel
    uint8_t *mtmp = (uint8_t *)c->d16a[0];
    uint8_t *stbuf = (uint8_t *)c->f64[0][0]; // sparse-table planes: <= 8 B / pixel
    int levels = 1;
    while ((1 << levels) <= plan.ksize) levels++;
    if (levels > 8) return set_err(c, RSM_E_INVALID, "erode size");
    for (int v = 0; v < 2; v++) {
        HIPCHK(c, hipMemcpyAsync(raw_img, in->image[v], opx * 3, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(raw_msk, in->mask[v], opx, hipMemcpyHostToDevice, st));
        const double *K = in->K[v];
        launch_rect_map(plan.ir[v], K[0], K[4], K[2], K[5], W, H, map1, map2, st);                 // :144
        launch_remap(raw_img, in->origin_width, in->origin_height, 3, map1, map2, W, H, c->img[top][v], st); // :154
        launch_remap(raw_msk, in->origin_width, in->origin_height, 1, map1, map2, W, H, mtmp, st);          // :156
        launch_erode_gray(mtmp, W, H, plan.ksize, c->d_j1, c->d_j2, stbuf, c->msk[top][v], st);             // :157-158
        HIPCHK(c, hipStreamSynchronize(st)); // raw buffers are reused by the next view
    }
    HIPCHK(c, hipGetLastError());
    memcpy(out->Q, plan.Q, sizeof plan.Q);
    memcpy(out->R_final, plan.R_final, sizeof plan.R_final);
    memcpy(out->T_final, plan.T_final, sizeof plan.T_final);
    for (int v = 0; v < 2; v++) {
        memcpy(out->P[v], plan.Pext[v], sizeof plan.Pext[v]);
        if (out->image[v]) HIPCHK(c, hipMemcpyAsync(out->image[v], c->img[top][v], px * 3, hipMemcpyDeviceToHost, st));
        if (out->mask[v]) HIPCHK(c, hipMemcpyAsync(out->mask[v], c->msk[top][v], px, hipMemcpyDeviceToHost, st));
    }
    out->width = W;
    out->height = H;
    HIPCHK(c, hipStreamSynchronize(st));
    s = upload_cloud_params(c);
    if (s != RSM_OK) return s;
    c->have_pair = true;
    c->have_result = false;
    return RSM_OK;
}
