// rsm_cloud.hip -- the cloud back end's host side: the per-pair filter, moving-least-squares smoothing and multi-view
// duplicate deletion (k_filter.hip, k_mls.hip, k_dedup.hip).  All three take their scratch from the context's filter arena.
#include "rsm_ctx.h"

#include <algorithm>
#include <cmath>
#include <string.h>

#include <vector>

// ---- per-pair cloud filter (CloudOptimization/CCloudOptimization.cpp:82-121) -------------------------------------
static int filter_params_ok(const rsm_filter_params *p) {
    return p && p->sor_mean_k >= 1 && p->sor_mean_k <= 100000 && p->normal_radius > 0.0 && p->sor_std_mul == p->sor_std_mul;
}

// the filter's buffers come from the context's arena: (re)sized for the cloud at hand, then the caller-visible ones first
static int filter_buffers(rsm_ctx *c, int64_t n, bool want_normals, float **dx, int32_t **dk, float **df, float4 **dn, size_t extra = 0) {
    if (!c->filt_arena) c->filt_arena = filter_arena_create();
    const size_t own = (size_t)n * (12 + 4 + 12 + 16) + 4096 + extra;
    if (filter_arena_reserve(c->filt_arena, own + filter_arena_bytes(n)) != RSM_OK)
        return set_err(c, RSM_E_NOMEM, "cloud filter: no device memory for %lld points", (long long)n);
    *dx = (float *)filter_arena_alloc(c->filt_arena, sizeof(float) * 3 * (size_t)n);
    *dk = (int32_t *)filter_arena_alloc(c->filt_arena, sizeof(int32_t) * (size_t)n);
    *df = (float *)filter_arena_alloc(c->filt_arena, sizeof(float) * 3 * (size_t)n);
    *dn = want_normals ? (float4 *)filter_arena_alloc(c->filt_arena, sizeof(float4) * (size_t)n) : nullptr;
    if (!*dx || !*dk || !*df || (want_normals && !*dn)) return set_err(c, RSM_E_NOMEM, "cloud filter: arena too small");
    return RSM_OK;
}

// ---- the radius outlier pass (CCloudOptimization.cpp:90-96; k_filter_outrem.hip): a setting of the context, because rsm_filter_params
// travels by pointer through four entries and cannot grow
// nullptr, or why the grid cannot take this search radius
static const char *outrem_radius_fault(double radius) {
    if (!std::isfinite(radius)) return "the radius is not finite";
    if (!(radius > 0.0)) return "the radius is not positive";
    if (!((float)radius > 0.0f)) return "the radius is 0 in float32"; // (the grid's cell edge)
    const float r2 = (float)(radius * radius);
    if (!(r2 > 0.0f)) return "the radius' square is 0 in float32";
    if (!std::isfinite(r2)) return "the radius' square is infinite in float32";
    return nullptr;
}
extern "C" int rsm_filter_set_outrem(rsm_ctx *c, const rsm_outrem_params *p) {
    if (!c) return RSM_E_INVALID;
    FilterOutrem &o = c->filt_route.outrem;
    if (!p) {
        o.on = false;
        return RSM_OK;
    }
    if (p->min_neighbors < 0) return set_err(c, RSM_E_INVALID, "rsm_filter_set_outrem: min_neighbors %d is negative", p->min_neighbors);
    if (const char *why = outrem_radius_fault(p->radius)) return set_err(c, RSM_E_INVALID, "rsm_filter_set_outrem: %s (%g)", why, p->radius);
    o.on = true;
    o.min_neighbors = p->min_neighbors;
    o.radius = p->radius;
    return RSM_OK;
}
extern "C" int rsm_filter_last_outrem(rsm_ctx *c, int64_t info[4]) {
    if (!c || !info) return RSM_E_INVALID;
    const FilterOutrem &o = c->filt_route.outrem;
    info[0] = o.points_in;
    info[1] = o.removed;
    info[2] = o.window;
    info[3] = o.nonfinite;
    return RSM_OK;
}
// a filter call that ends before filter_cloud_device (an empty cloud) leaves the report of a pass that had nothing to do
static void outrem_report_empty(rsm_ctx *c) {
    FilterOutrem &o = c->filt_route.outrem;
    o.points_in = o.on ? 0 : -1;
    o.removed = o.nonfinite = 0;
    o.window = 0;
}

extern "C" int rsm_stage_radius_count(rsm_ctx *c, const float *xyz, int64_t n, double radius, int cap, int32_t *count) {
    if (!c || n < 0 || n > (int64_t)INT32_MAX || (n > 0 && (!xyz || !count))) return RSM_E_INVALID;
    if (cap < 1) return set_err(c, RSM_E_INVALID, "rsm_stage_radius_count: cap %d is below 1", cap);
    if (const char *why = outrem_radius_fault(radius)) return set_err(c, RSM_E_INVALID, "rsm_stage_radius_count: %s (%g)", why, radius);
    HIPCHK(c, hipSetDevice(c->device));
    if (n == 0) return RSM_OK;
    Tmp t(c);
    if (!c->filt_arena) c->filt_arena = filter_arena_create();
    if (filter_arena_reserve(c->filt_arena, (size_t)n * 16 + 4096 + filter_arena_bytes(n)) != RSM_OK)
        return set_err(c, RSM_E_NOMEM, "rsm_stage_radius_count: no device memory for %lld points", (long long)n);
    float *dx = (float *)filter_arena_alloc(c->filt_arena, sizeof(float) * 3 * (size_t)n);
    int32_t *dc = (int32_t *)filter_arena_alloc(c->filt_arena, sizeof(int32_t) * (size_t)n);
    if (!dx || !dc) return set_err(c, RSM_E_NOMEM, "rsm_stage_radius_count: arena too small");
    HIPCHK(c, hipMemcpyAsync(dx, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const int s = radius_count_device(c->filt_arena, dx, n, radius, cap, dc, c->stream);
    if (s != RSM_OK) return set_err(c, s, "rsm_stage_radius_count failed");
    t.down(count, (const int32_t *)dc, (size_t)n);
    return finish(c, t);
}

extern "C" int rsm_filter_cloud(rsm_ctx *c, const float *xyz, int64_t n, const rsm_filter_params *prm, int32_t *kept_index,
                                float *normals, int64_t *n_kept, double *stats) {
    if (!c || n < 0 || (n > 0 && (!xyz || !kept_index)) || !n_kept || !filter_params_ok(prm)) return RSM_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    *n_kept = 0;
    if (n == 0) {
        outrem_report_empty(c);
        return RSM_OK;
    }
    Tmp t(c);
    float *dx, *df;
    int32_t *dk;
    float4 *dn;
    const int sb = filter_buffers(c, n, normals != nullptr, &dx, &dk, &df, &dn);
    if (sb != RSM_OK) return sb;
    HIPCHK(c, hipMemcpyAsync(dx, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const int s = filter_cloud_device(c->filt_arena, dx, n, prm->sor_mean_k, prm->sor_std_mul, prm->normal_radius, prm->cam_center, dk, df, dn,
                                      n_kept, stats, c->stream, nullptr, &c->filt_route);
    if (s != RSM_OK) return set_err(c, s, "cloud filter failed");
    if (*n_kept > 0) {
        t.down(kept_index, (const int32_t *)dk, (size_t)*n_kept);
        if (normals) t.down(normals, (const float *)dn, (size_t)4 * *n_kept);
    }
    return finish(c, t);
}

// The stream of the per-pair cloud filter.  With several pairs in flight on a GPU the filter of one pair runs beside the matching of
// the others, and its large kernels (21 000 workgroups of 75 KB LDS) took the compute units the matchers' dependent launches -- the
// top level's refine sweeps, the loop's critical path -- were waiting for: 29.5 ms per pair in the adapter's loop for 15.3 ms of
// matching + 9.5 ms of filter.  On a stream of the lowest priority the dispatcher hands compute units to the matchers first.
static hipStream_t filter_stream(rsm_ctx *c) {
    if (!c->opt_filter_low_priority) return c->stream;
    if (!c->stream_filter) {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || hipStreamCreateWithPriority(&c->stream_filter, hipStreamNonBlocking, least) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_filter, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (c->stream_filter) (void)hipStreamDestroy(c->stream_filter);
            c->stream_filter = nullptr;
            return c->stream;
        }
    }
    if (hipEventRecord(c->ev_filter, c->stream) != hipSuccess || hipStreamWaitEvent(c->stream_filter, c->ev_filter, 0) != hipSuccess) return c->stream;
    return c->stream_filter;
}

// A cloud as the depth map launch_cloud made it, on the device: what the per-pair filter needs beside the points themselves.
struct DepthCloud {
    const uint8_t *flags;      // k_cloud's per-pixel "emitted a point" flags, W bytes a row
    const int64_t *row_offset; // ... and its per-row offsets (first row: box.YL)
    int W, H;                  // the level's size
    Mg box;                    // the margin's box
    const double *xyz;         // the n fp64 points in compaction order
    int64_t n;
    double qz;                 // Q[2][3] * scale (.cpp:698)
    const double *R, *T;       // R_final, T_final (host)
};
// The filter's device buffers of one call (the context's arena: valid until its next reserve) and the stream the call ran on
struct FilteredCloud {
    float *xyz;         // the n unfiltered float32 points
    int32_t *kept;      // first m valid
    float4 *normals;    // first m valid (nullptr: not asked for)
    int64_t m;
    hipStream_t stream;
};

// From "fill the FilterLattice" to the info fields: the filter of a depth-map cloud, behind rsm_filter_last_cloud (the cloud of the last
// rsm_run_pair) and rsm_stage_filter_depth_map (the cloud of a given disparity map).  Every "filter_*" option and every rsm_filter_last_*
// report behaves the same behind either.
static int filter_depth_cloud(rsm_ctx *c, const rsm_filter_params *prm, const DepthCloud &dc, bool want_normals, FilteredCloud *out, double *stats) {
    const int64_t n = dc.n;
    float *dx, *df;
    int32_t *dk;
    float4 *dn;
    // The cloud is a depth map: its pixel lattice (k_cloud's flags and row offsets are still in place)
    // decides most k-nearest queries (k_filter_win.hip: k_sor_window).  Needs R_final to be a rotation (distances in the cloud =
    // distances in the camera frame); anything else takes the generic search.
    const Mg &mg = dc.box;
    FilterLattice lat{};
    bool use_lat = c->opt_filter_window && mg.XR >= mg.XL && mg.YR >= mg.YL;
    if (use_lat) {
        const double *R = dc.R;
        for (int i = 0; i < 3 && use_lat; i++)
            for (int j = 0; j < 3; j++) {
                double d = 0.0;
                for (int l = 0; l < 3; l++) d += R[3 * l + i] * R[3 * l + j];
                if (!(fabs(d - (i == j ? 1.0 : 0.0)) < 1e-9)) use_lat = false;
            }
        lat.flags = dc.flags;
        lat.row_offset = dc.row_offset;
        lat.W = dc.W;
        lat.XL = mg.XL, lat.XR = mg.XR, lat.YL = mg.YL, lat.YR = mg.YR;
        lat.xyz64 = dc.xyz;
        lat.qz = dc.qz;
        memcpy(lat.R, dc.R, sizeof lat.R);
        memcpy(lat.T, dc.T, sizeof lat.T);
        if (!(fabs(lat.qz) > 0.0) || !std::isfinite(lat.qz)) use_lat = false;
    }
    int left = -1, tile_left = -1;
    lat.undecided_out = &left;
    lat.tile_left_out = &tile_left;
    lat.list_pass = c->opt_filter_list;
    lat.wg_max = c->opt_filter_wg_max;
    lat.normals_wmax = std::min(c->opt_filter_normals_window, 40);
    c->filt_normals[0] = 0, c->filt_normals[1] = -1;
    lat.normals_out = c->filt_normals;
    c->filt_passes = FilterPasses{};
    lat.passes_out = &c->filt_passes;
    int used_radius = 0;
    lat.radius_out = &used_radius;
    lat.radius = c->opt_filter_window <= 1 ? 0 : (c->opt_filter_window <= 7 ? 7 : (c->opt_filter_window <= 12 ? 12 : (c->opt_filter_window <= 16 ? 16 : (c->opt_filter_window <= 20 ? 20 : 24))));
    // The probed radius is a property of the rig (how thick its clouds are in pixel spacings): a context remembers what the probe
    // chose for its last cloud and skips the three probe launches and their host round trips (0.6 ms of C2's 14.8) while the
    // choice keeps deciding most queries; every 8th call, a different k, a different image size or a set_option probes again.
    const bool memo_ok = c->opt_filter_window == 1 && c->filt_memo_radius > 0 && c->filt_memo_k == prm->sor_mean_k && c->filt_memo_w == dc.W &&
                         c->filt_memo_h == dc.H && c->filt_memo_uses < 7;
    if (use_lat && memo_ok) lat.radius = c->filt_memo_radius;
    const int sb = filter_buffers(c, n, want_normals, &dx, &dk, &df, &dn, use_lat ? cloud_lattice_bytes(mg.XL, mg.XR, mg.YL, mg.YR) + (size_t)n * 4 + 8192 : 0);
    if (sb != RSM_OK) return sb;
    const hipStream_t fs = filter_stream(c);
    launch_f64_to_f32x3(dc.xyz, n, dx, fs); // InsertPoint's cast, CCloudOptimization.cpp:61
    int64_t m = 0;
    const int s = filter_cloud_device(c->filt_arena, dx, n, prm->sor_mean_k, prm->sor_std_mul, prm->normal_radius, prm->cam_center, dk, df, dn, &m, stats,
                                      fs, use_lat ? &lat : nullptr, &c->filt_route);
    if (s != RSM_OK) return set_err(c, s, "cloud filter failed");
    if (use_lat && c->opt_filter_window == 1) {
        if (memo_ok && tile_left >= 0 && (double)tile_left <= 0.3 * (double)n) c->filt_memo_uses++; // still a good choice
        else if (!memo_ok && used_radius > 0) { // a fresh probe's choice
            c->filt_memo_radius = used_radius;
            c->filt_memo_k = prm->sor_mean_k;
            c->filt_memo_w = dc.W;
            c->filt_memo_h = dc.H;
            c->filt_memo_uses = 0;
        } else c->filt_memo_radius = 0; // left too much over (or no window at all): probe next time
    }
    c->filt_info[0] = left >= 0 ? used_radius : 0;
    c->filt_info[1] = left >= 0 ? left : 0;
    c->filt_tile_left = tile_left >= 0 ? tile_left : 0;
    c->filt_info[2] = n;
    c->filt_info[3] = m;
    *out = FilteredCloud{dx, dk, dn, m, fs};
    return RSM_OK;
}

extern "C" int rsm_filter_last_cloud(rsm_ctx *c, const rsm_filter_params *prm, rsm_point16 *d_points, float *d_normals,
                                     int64_t max_points, int64_t *n_kept, double *stats) {
    if (!c || !n_kept || !filter_params_ok(prm)) return RSM_E_INVALID;
    if (!c->have_result) return set_err(c, RSM_E_STATE, "no result");
    HIPCHK(c, hipSetDevice(c->device));
    *n_kept = 0;
    const int64_t n = c->n_points;
    if (n == 0) {
        outrem_report_empty(c);
        return RSM_OK;
    }
    Tmp t(c);
    // the cloud is the depth map this context just made
    const int k = c->N - 1;
    const double scale = (double)c->Wk[0] / c->in.origin_width * (1 << k); // .cpp:692
    const DepthCloud dc{c->cloud_flags, c->row_offset, c->Wk[k], c->Hk[k], c->mg[k][0], c->xyz, n, c->in.Q[11] * scale, c->in.R_final, c->in.T_final};
    FilteredCloud f{};
    const int s = filter_depth_cloud(c, prm, dc, d_normals != nullptr, &f, stats);
    if (s != RSM_OK) return s;
    const int64_t m = f.m;
    if (m > max_points) return set_err(c, RSM_E_INVALID, "rsm_filter_last_cloud: %lld points survive, capacity %lld", (long long)m, (long long)max_points);
    if (m > 0 && d_points) launch_pack_filtered16(c->xyz, c->bgr, f.kept, m, d_points, f.stream);
    if (m > 0 && d_normals) HIPCHK(c, hipMemcpyAsync(d_normals, f.normals, sizeof(float4) * (size_t)m, hipMemcpyDeviceToDevice, f.stream));
    *n_kept = m;
    if (f.stream != c->stream) HIPCHK(c, hipStreamSynchronize(f.stream));
    return finish(c, t);
}

// DisparityToCloud of a given top-level disparity map (rsm_stage_cloud's part) and the per-pair filter of that cloud, exactly as
// rsm_filter_last_cloud filters the cloud of a matched pair: no matching runs, so a test can put a lattice of any width in front of the filter.
extern "C" int rsm_stage_filter_depth_map(rsm_ctx *c, const double *disp, const uint8_t *mask_org, const uint8_t *img_own, int W, int H, const double *Q,
                                          double scale, const double *R_final, const double *T_final, const rsm_boundary *own,
                                          const rsm_filter_params *prm, float *xyz, int32_t *kept_index, float *normals, int64_t max_points,
                                          int64_t *n_points, int64_t *n_kept, double *stats) {
    if (!stage_ok(c, W, H) || !disp || !mask_org || !img_own || !Q || !R_final || !T_final || !own || !n_points || !n_kept || !filter_params_ok(prm) ||
        max_points < 0 || (max_points > 0 && (!xyz || !kept_index)))
        return RSM_E_INVALID;
    const Mg box = to_mg(*own);
    if (box.XL < 0 || box.YL < 0 || box.XR >= W || box.YR >= H) return RSM_E_INVALID;
    *n_points = *n_kept = 0;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    const int ksize = (int)ceil(0.02 * H);
    if (ksize < 1 || ksize > 4096) return RSM_E_INVALID;
    std::vector<int> j1, j2;
    ellipse_spans(ksize, j1, j2);
    double q[16];
    memcpy(q, Q, sizeof q);
    for (int i = 0; i < 4; i++) q[i * 4 + 3] *= scale;
    double *dd = t.up(disp, px);
    uint8_t *dm = t.up(mask_org, px);
    uint8_t *di = t.up(img_own, px * 3);
    int *d1 = t.up(j1.data(), (size_t)ksize), *d2 = t.up(j2.data(), (size_t)ksize);
    double *dq = t.up(q, 16), *dR = t.up(R_final, 9), *dT = t.up(T_final, 3);
    int32_t *pre = t.alloc<int32_t>((size_t)(W + 1) * H);
    int32_t *rc = t.alloc<int32_t>((size_t)H);
    int64_t *ro = t.alloc<int64_t>((size_t)H);
    int64_t *dn = t.alloc<int64_t>(1);
    uint8_t *fl = t.alloc<uint8_t>(px + CLOUD_BLOCKS(W, H));
    double *dx = max_points ? t.alloc<double>((size_t)max_points * 3) : nullptr;
    if (!t.ok) return finish(c, t);
    launch_bad_prefix(dm, W, H, pre, c->stream);
    launch_bad_blocks(pre, W, H, fl + px, c->stream);
    launch_cloud(dd, pre, di, W, H, ksize, d1, d2, dq, dR, dT, box, fl, fl + px, rc, ro, dn, dx, nullptr, max_points, c->stream);
    int64_t n = 0;
    t.down(&n, (const int64_t *)dn, 1);
    if (!t.ok) return finish(c, t);
    *n_points = n;
    if (n > max_points) return set_err(c, RSM_E_INVALID, "rsm_stage_filter_depth_map: %lld points, capacity %lld", (long long)n, (long long)max_points);
    if (n == 0) {
        outrem_report_empty(c);
        return finish(c, t);
    }
    const DepthCloud dc{fl, ro, W, H, box, dx, n, Q[11] * scale, R_final, T_final};
    FilteredCloud f{};
    const int s = filter_depth_cloud(c, prm, dc, normals != nullptr, &f, stats);
    if (s != RSM_OK) return s;
    if (f.stream != c->stream) HIPCHK(c, hipStreamSynchronize(f.stream));
    t.later(xyz, (const float *)f.xyz, (size_t)n * 3).later(kept_index, (const int32_t *)f.kept, (size_t)f.m).later(normals, (const float *)f.normals, (size_t)f.m * 4);
    *n_kept = f.m;
    return finish(c, t);
}

// What the passes behind the tile pass of the last rsm_filter_last_cloud[_host] / rsm_stage_filter_depth_map did
extern "C" int rsm_filter_last_passes(rsm_ctx *c, int64_t head[4], int64_t *passes, int64_t max_passes, int64_t *n_passes) {
    if (!c || !head || !n_passes || max_passes < 0 || (max_passes > 0 && !passes)) return RSM_E_INVALID;
    const FilterPasses &P = c->filt_passes;
    head[0] = P.ladder_in;
    head[1] = P.whole_in;
    head[2] = P.whole_over_lattice;
    head[3] = FILTER_MAX_PASSES;
    *n_passes = P.n;
    for (int i = 0; i < P.n && i < max_passes; i++) {
        passes[4 * i] = P.radius[i];
        passes[4 * i + 1] = P.entered[i];
        passes[4 * i + 2] = P.decided[i];
        passes[4 * i + 3] = P.workgroup[i];
    }
    return RSM_OK;
}

extern "C" int rsm_filter_last_normals_info(rsm_ctx *c, int64_t info[2]) {
    if (!c || !info) return RSM_E_INVALID;
    info[0] = c->filt_normals[0];
    info[1] = c->filt_normals[1];
    return RSM_OK;
}

extern "C" int rsm_filter_last_info(rsm_ctx *c, int64_t info[4]) {
    if (!c || !info) return RSM_E_INVALID;
    memcpy(info, c->filt_info, sizeof c->filt_info);
    return RSM_OK;
}

extern "C" int rsm_filter_last_grid(rsm_ctx *c, double grid[4], int64_t info[6]) {
    if (!c || !grid || !info) return RSM_E_INVALID;
    const FilterRoute &r = c->filt_route;
    grid[0] = r.h;
    for (int a = 0; a < 3; a++) {
        grid[1 + a] = r.origin[a];
        info[a] = r.cells[a];
    }
    info[3] = r.levels;
    info[4] = r.kind0;
    info[5] = r.kinds;
    return RSM_OK;
}

extern "C" int rsm_filter_last_cloud_host(rsm_ctx *c, const rsm_filter_params *prm, rsm_point16 *h_points, float *h_normals,
                                          int64_t max_points, int64_t *n_kept, double *stats) {
    if (!c || !n_kept || !h_points || max_points < 0) return RSM_E_INVALID;
    if (!c->have_result) return set_err(c, RSM_E_STATE, "no result");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->pack16) {
        const int s = dalloc(c, &c->pack16, c->cap_px);
        if (s != RSM_OK) return s;
    }
    if (h_normals && !c->pack_nrm) {
        const int s = dalloc(c, &c->pack_nrm, c->cap_px * 4);
        if (s != RSM_OK) return s;
    }
    const int64_t cap = (int64_t)c->cap_px < max_points ? (int64_t)c->cap_px : max_points;
    const int s = rsm_filter_last_cloud(c, prm, c->pack16, h_normals ? c->pack_nrm : nullptr, cap, n_kept, stats);
    if (s != RSM_OK) return s;
    const size_t m = (size_t)*n_kept;
    if (m > 0) {
        HIPCHK(c, hipMemcpyAsync(h_points, c->pack16, m * sizeof(rsm_point16), hipMemcpyDeviceToHost, c->stream));
        if (h_normals) HIPCHK(c, hipMemcpyAsync(h_normals, c->pack_nrm, m * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return RSM_OK;
}

// ---- moving-least-squares smoothing (CCloudOptimization::run, CloudOptimization/CCloudOptimization.cpp:348-389) -----------
static int mls_args_ok(rsm_ctx *c, int64_t n, const rsm_mls_params *p, const void *out_xyz, const void *out_nrm, const void *src_index,
                       const int64_t *n_out) {
    return c && p && n_out && out_xyz && out_nrm && src_index && n >= 0 && n <= (int64_t)INT32_MAX && std::isfinite(p->search_radius) &&
           p->search_radius > 0.0 && p->polynomial_order >= 0 && p->polynomial_order <= 2;
}
// (re)sizes the context's filter arena to `bytes` for an MLS ("mls") or duplicate-deletion ("dedup") call on n points
static int arena_reserve(rsm_ctx *c, const char *who, int64_t n, size_t bytes) {
    if (!c->filt_arena) c->filt_arena = filter_arena_create();
    if (filter_arena_reserve(c->filt_arena, bytes) != RSM_OK) return set_err(c, RSM_E_NOMEM, "%s: no device memory for %lld points", who, (long long)n);
    return RSM_OK;
}

extern "C" int rsm_mls_cloud_device(rsm_ctx *c, const rsm_point16 *d_points, int64_t n, const float *d_ref_normals, const rsm_mls_params *p,
                                    float *d_out_xyz, float *d_out_normals, int32_t *d_src_index, int64_t *n_out) {
    if (!mls_args_ok(c, n, p, d_out_xyz, d_out_normals, d_src_index, n_out) || (n > 0 && !d_points)) return RSM_E_INVALID;
    *n_out = 0;
    if (n == 0) return RSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int s = arena_reserve(c, "mls", n, sizeof(float) * 3 * (size_t)n + 4096 + mls_arena_bytes(n));
    if (s != RSM_OK) return s;
    float *dx = (float *)filter_arena_alloc(c->filt_arena, sizeof(float) * 3 * (size_t)n);
    if (!dx) return set_err(c, RSM_E_NOMEM, "mls: arena too small");
    launch_point16_xyz(d_points, n, dx, c->stream);
    s = mls_cloud_device(c->filt_arena, dx, n, (const float4 *)d_ref_normals, p->search_radius, p->polynomial_order, d_out_xyz, d_out_normals,
                         d_src_index, n_out, c->stream);
    if (s != RSM_OK) return set_err(c, s, "mls failed");
    return RSM_OK;
}

extern "C" int rsm_mls_cloud(rsm_ctx *c, const float *xyz, int64_t n, const float *ref_normals, const rsm_mls_params *p, float *out_xyz,
                             float *out_normals, int32_t *src_index, int64_t *n_out) {
    if (!mls_args_ok(c, n, p, out_xyz, out_normals, src_index, n_out) || (n > 0 && !xyz)) return RSM_E_INVALID;
    *n_out = 0;
    if (n == 0) return RSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bx = sizeof(float) * 3 * (size_t)n, bn = sizeof(float) * 4 * (size_t)n, bi = sizeof(int32_t) * (size_t)n;
    int s = arena_reserve(c, "mls", n, 2 * bx + (ref_normals ? bn : 0) + bn + bi + 5 * 256 + 4096 + mls_arena_bytes(n));
    if (s != RSM_OK) return s;
    FilterArena *A = c->filt_arena;
    float *dx = (float *)filter_arena_alloc(A, bx), *dox = (float *)filter_arena_alloc(A, bx), *don = (float *)filter_arena_alloc(A, bn);
    int32_t *doi = (int32_t *)filter_arena_alloc(A, bi);
    float *dr = ref_normals ? (float *)filter_arena_alloc(A, bn) : nullptr;
    if (!dx || !dox || !don || !doi || (ref_normals && !dr)) return set_err(c, RSM_E_NOMEM, "mls: arena too small");
    HIPCHK(c, hipMemcpyAsync(dx, xyz, bx, hipMemcpyHostToDevice, c->stream));
    if (dr) HIPCHK(c, hipMemcpyAsync(dr, ref_normals, bn, hipMemcpyHostToDevice, c->stream));
    s = mls_cloud_device(A, dx, n, (const float4 *)dr, p->search_radius, p->polynomial_order, dox, don, doi, n_out, c->stream);
    if (s != RSM_OK) return set_err(c, s, "mls failed");
    const size_t m = (size_t)*n_out;
    if (m > 0) {
        HIPCHK(c, hipMemcpyAsync(out_xyz, dox, sizeof(float) * 3 * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(out_normals, don, sizeof(float) * 4 * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(src_index, doi, sizeof(int32_t) * m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return RSM_OK;
}

// ---- multi-view duplicate deletion (the isdelete branch of CCloudOptimization::run, CCloudOptimization.cpp:152-346) ----------------
static int dedup_args_ok(rsm_ctx *c, int64_t n, const rsm_dedup_view *v, int np, const void *index, const int64_t *n_out, const int64_t *stats) {
    if (!c || !index || !n_out || !stats || n < 0 || n > (int64_t)INT32_MAX) return 0;
    if (n > 0 && (np < 1 || !v)) return 0;
    return np < 1 || (v && dedup_views_ok(v, np));
}

extern "C" int rsm_dedup_cloud_device(rsm_ctx *c, const rsm_point16 *d_points, const float *d_normals4, int64_t n, const rsm_dedup_view *views,
                                      int n_pairs, int32_t *d_index, rsm_point16 *d_out_points, float *d_out_normals, int64_t *n_out,
                                      int64_t stats[4]) {
    if (!dedup_args_ok(c, n, views, n_pairs, d_index, n_out, stats) || (n > 0 && (!d_points || !d_normals4))) return RSM_E_INVALID;
    *n_out = 0;
    for (int t = 0; t < 4; t++) stats[t] = 0;
    if (n == 0) return RSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int s = arena_reserve(c, "dedup", n, 4096 + dedup_arena_bytes(views, n_pairs, n));
    if (s != RSM_OK) return s;
    s = dedup_cloud_device(c->filt_arena, (const float *)d_points, 4, (const float4 *)d_normals4, n, views, n_pairs, d_index, n_out, stats, c->stream);
    if (s != RSM_OK) return set_err(c, s, "dedup failed");
    if (*n_out > 0 && (d_out_points || d_out_normals)) {
        launch_dedup_gather(d_points, d_normals4, d_index, *n_out, d_out_points, d_out_normals, c->stream);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipGetLastError());
    }
    return RSM_OK;
}

extern "C" int rsm_dedup_cloud(rsm_ctx *c, const float *xyz, const float *normals4, int64_t n, const rsm_dedup_view *views, int n_pairs,
                               int32_t *index, int64_t *n_out, int64_t stats[4]) {
    if (!dedup_args_ok(c, n, views, n_pairs, index, n_out, stats) || (n > 0 && (!xyz || !normals4))) return RSM_E_INVALID;
    *n_out = 0;
    for (int t = 0; t < 4; t++) stats[t] = 0;
    if (n == 0) return RSM_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bx = sizeof(float) * 3 * (size_t)n, bn = sizeof(float) * 4 * (size_t)n, bi = sizeof(int32_t) * (size_t)n;
    int s = arena_reserve(c, "dedup", n, bx + bn + bi + 3 * 256 + 4096 + dedup_arena_bytes(views, n_pairs, n));
    if (s != RSM_OK) return s;
    FilterArena *A = c->filt_arena;
    float *dx = (float *)filter_arena_alloc(A, bx), *dn = (float *)filter_arena_alloc(A, bn);
    int32_t *di = (int32_t *)filter_arena_alloc(A, bi);
    if (!dx || !dn || !di) return set_err(c, RSM_E_NOMEM, "dedup: arena too small");
    HIPCHK(c, hipMemcpyAsync(dx, xyz, bx, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dn, normals4, bn, hipMemcpyHostToDevice, c->stream));
    s = dedup_cloud_device(A, dx, 3, (const float4 *)dn, n, views, n_pairs, di, n_out, stats, c->stream);
    if (s != RSM_OK) return set_err(c, s, "dedup failed");
    if (*n_out > 0) {
        HIPCHK(c, hipMemcpyAsync(index, di, sizeof(int32_t) * (size_t)*n_out, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return RSM_OK;
}
