// rsm_dev.h -- internal declarations shared by the HIP translation units of librsm_mi355.so.
// gfx950 (MI355X) only: wave = 64 lanes, no portability layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "refine_plan.h" // Mg, refine_interior / refine_skew_strips / refine_skew_fits: the launchers and the schedule share them

#define NOMATCH (-10000) // reconstruction/CStereoMatching.h:9
#define WAVE 64
#define RF_MAX_SWEEPS 1024
#define RF_NOKEY ((int16_t)-32768)
#define RF_NOKEY2 0x80008000u // both ways of DirArgs::rf_key empty
#define RF_PPT 4      // pixels per thread of the refine sweep kernel
#define RF_TILE_MAXT 8 // sweeps per launch of the tile kernel (k_refine_tile), at most
#define SBV_S 32 // SetBoundary: row segments per column of the vertical sweeps
// What a row segment of a column does to the (bl, br) pair the vertical sweep carries through it (k_setb_vert): bl -> max(bl + a_bl, c_bl),
// br -> min(br + a_br, c_br); sav_l / sav_r: the downward sweep's pair at the row above the segment, saved for the upward sweep
struct SbvRec {
    int a_bl, c_bl, a_br, c_br, sav_l, sav_r;
};
static_assert(sizeof(SbvRec) == 24, "SbvRec: six ints");
// int32 scratch of launch_set_boundary (in rf_list), per direction: [SBV_S][W] records, then the pair the downward sweep ended with, [W][2]
#define SETB_SCRATCH(W) ((size_t)(SBV_S * (sizeof(SbvRec) / sizeof(int)) + 2) * (size_t)(W))

// Everything one direction of one stage may need. Direction v: own view = v, other = 1-v
// (IsZeroOne = (v == 0) in the reference's signatures).
struct DirArgs {
    const uint8_t *img_own, *img_oth;   // BGR interleaved, stride 3*W
    const uint32_t *img4_own, *img4_oth; // BGRX copies (one dword per pixel), stride W
    const uint8_t *mask_own, *mask_oth; // stride W
    const int32_t *S1_own, *S2_own;     // (2r+1)^2*3 window sums of bytes / squared bytes, centre-indexed
    const int32_t *S1_oth, *S2_oth;
    Mg own, oth;
    int16_t *d16_in, *d16_out; // int16 disparity maps (in may alias out when the stage allows it)
    int16_t *BL, *BR;          // candidate intervals (absolute columns)
    const double *parent;      // fp64 disparity of level k-1 (this direction)
    const int32_t *parent_nv;  // next-valid-column table of `parent`
    double *f64_a, *f64_b;     // fp64 disparity ping-pong / uniqueness maps
    uint32_t *rf_key;          // refine cache, per pixel: iMatch - x = int(d - 1.5) of the entry in way 0 (low half) | way 1 (high half), RF_NOKEY = empty
    double2 *rf_ent;           // refine cache, [way * rf_stride + pixel]: the data term (pwp, delta = pdp - dCenter) of that iMatch
};

// A data-term cache entry computed inside a k_refine_skew launch, applied to the cache by k_refine_apply after it.
struct RfUpd {
    uint32_t pix; // pixel index | direction << 31
    int32_t rel;  // iMatch - x of the entry (its parity selects the way)
    double pwp, delta;
};
#define RF_UPD_SHARDS 32 // append counters (one counter serialises at ~88 appends per microsecond)

// ints of StageArgs::wrow for a level of H rows: [0, 2H) wide pixels per (direction, row) appended by k_ncc_dot4; then two row lists of
// 2 (H + 1) ints (k_ncc_rowgemm's, k_ncc_slide's); then [2H] pixels with an interval longer than ncc_mid and [2H] the widest interval, per
// (direction, row), from k_ncc_rowstat
#define NCC_WROW_INTS(H) (10 * (H) + 32)
#define NCC_WROW_LIST(H, which) (2 * (H) + (which) * (2 * (H) + 2))
#define NCC_WROW_MID(H) (6 * (H) + 4)
#define NCC_WROW_MAX(H) (8 * (H) + 4)

struct StageArgs {
    DirArgs d[2];
    int ndir;    // 1 or 2 (gridDim.z)
    int W, H;    // this level
    int Wp, Hp;  // parent level
    int r;       // MatchBlockRadius
    int offset;  // m_offset
    double ws;   // m_ws
    int flag;    // stage-specific (refine: the top level)
    size_t rf_stride;  // refine: elements between the two cache ways (>= W*H)
    RfUpd *upd_list;   // refine (k_refine_skew, k_refine_tile): RF_UPD_SHARDS regions of upd_cap records
    int32_t *upd_cnt;  // [2][RF_UPD_SHARDS]: append counters, the set in use alternates per launch (rf_launch & 1)
    int upd_cap;
    int rf_launch;     // refine (k_refine_skew, k_refine_tile, k_refine_apply): index of the multi-sweep launch within the level
    int rf_no_prefill; // refine (k_refine_first): leave the second cache way empty (option refine_prefill = 0)
    int rf_rekey_far;  // refine (k_refine_rekey): predict the neighbour key on the far side of the interval (tests)
    int skew_rows;     // refine (k_refine_skew): rows per chunk
    int skew_uw;       // refine (k_refine_skew): columns a strip owns (<= 66 - 2T)
    int skew_prio;     // refine (k_refine_skew): issue priority rotates every 2^skew_prio shader clocks (0: never)
    int opt_ncc_bytes;              // force the generic byte-wise NCC kernel (A/B validation)
    int opt_no_exact;               // skip k_ncc_exact (timing A/B only: ties then follow the integer form)
    uint32_t *rf_list; // NCC: worklist of wide pixels (dir << 31 | pixel index); SetBoundary: segment-map scratch
    uint32_t *tie_list; // NCC: pixels (dir << 31 | pixel index) whose scan saw a (near) tie -> k_ncc_exact
    int32_t *tie_cnt;   // NCC: [0] entries of tie_list after an initial-match launch, [1] after a Rematch launch (zero on entry)
    int32_t *wrow;     // NCC: [dir * H + y] wide pixels of a row after k_ncc_dot4 (zero on entry); rows with many go to k_ncc_rowgemm
    int opt_no_rowgemm; // A/B: every wide pixel through k_ncc_wide
    int ncc_mid;        // NCC: in a row with many pixels of long intervals, every interval longer than this joins the row kernels (<= NCC_WIDE = 160, the band kernel's limit)
    int ncc_slide_max;  // NCC: rows whose widest interval is at most this take k_ncc_slide, the others k_ncc_rowgemm
    int32_t *ncc_cnt;  // NCC: [0] number of wide pixels in rf_list (zero before an initial-match launch), [16 + dir * H + y] Rematch pixels of a row
};

// rows and columns of one margin, and of the larger margin over a stage's directions: what a launch over the margins covers
struct Extent {
    int rows, cols;
};
inline Extent margin_extent(const Mg &m) { return Extent{m.YR - m.YL + 1, m.XR - m.XL + 1}; }
inline Extent margin_extent(const StageArgs &a) {
    Extent e{0, 0};
    for (int v = 0; v < a.ndir; v++) {
        const Extent d = margin_extent(a.d[v].own);
        e = Extent{std::max(e.rows, d.rows), std::max(e.cols, d.cols)};
    }
    return e;
}

// ---- launchers (each enqueues on `st`, no sync) ----------------------------------------------
void launch_fill_i16(int16_t *p, size_t n, int16_t v, hipStream_t st);
void launch_fill_f64(double *p, size_t n, double v, hipStream_t st);
void launch_fill_i32(int32_t *p, size_t n, int32_t v, hipStream_t st);
void launch_pyr_down(const uint8_t *src, int W, int H, int C, uint8_t *dst, hipStream_t st);
// out4 = {XL, XR, YL, YR} initialised by the kernel launcher (inverted defaults, .cpp:1014-1017)
void launch_find_margin(const uint8_t *mask, int W, int H, int r, int *out4, hipStream_t st);
void launch_find_margin_batch(int n, const uint8_t *const *masks, const int *Ws, const int *Hs, int r, int *out4, int *h_init,
                              hipStream_t st);
void launch_bgr_to_bgrx(const uint8_t *img, int W, int H, uint32_t *out, hipStream_t st);
void launch_box_sums(const uint32_t *img4, int W, int H, int r, int32_t *tmp1, int32_t *tmp2,
                     int32_t *S1, int32_t *S2, hipStream_t st);

void launch_next_valid(const double *parent, int Wp, int Hp, int32_t *nv, hipStream_t st);
void launch_next_valid2(const double *parent0, const double *parent1, int Wp, int Hp, int32_t *nv0, int32_t *nv1, hipStream_t st);
void launch_hl_interval(const StageArgs &a, hipStream_t st);
// mode 0: lowest level (interval = other margin), 1: interval arrays BL/BR into NOMATCH-filled out,
// 2: rematch (only pixels whose d16_in is NOMATCH; in place; the pixels come from launch_set_boundary(.., true))
void launch_ncc_argmax(const StageArgs &a, int mode, hipStream_t st);

void launch_smooth(const StageArgs &a, hipStream_t st, bool copy_outside = true); // d16_in -> d16_out
hipError_t launch_order(const StageArgs &a, hipStream_t st);   // d16_in in place; an error: nothing was launched
void launch_uniq_s16(int16_t *p, const int16_t *q, int W, int H, Mg own, Mg oth, hipStream_t st);
void launch_uniq_f64(double *p, const double *q, int W, int H, Mg own, Mg oth, hipStream_t st);
// d16_in, mask_own -> BL, BR; emit_list: also fill rf_list / ncc_cnt with the pixels Rematch has to evaluate
void launch_set_boundary(const StageArgs &a, hipStream_t st, bool emit_list = false);
void launch_median(const StageArgs &a, hipStream_t st);        // d16_in -> d16_out (pre-filled NOMATCH)
void launch_exp_neg(const double *t, double *out, long long n, hipStream_t st, int small_form); // the specified exp(-t) (tests)
// k_refine_skew's division without operand scaling beside the compiler's a / b (tests)
void launch_refine_xi(const uint32_t *A, const uint32_t *B, int W, int H, int form, double *out, hipStream_t st); // the data term's matching costs (tests)
void launch_sqrt_check(unsigned int first, long long n, unsigned long long *mismatches, hipStream_t st); // k_filter.hip: knn_select.h's sqrtf_rn on the device
void launch_win_index_check(int ncx, int ncy, unsigned long long *mismatches, hipStream_t st);            // k_filter.hip: win_index.h on the device
void launch_div_unscaled(const double *a, const double *b, double *q_fast, double *q_ieee, long long n, hipStream_t st);
void launch_refine_init(const StageArgs &a, hipStream_t st);   // d16_in -> f64_a, f64_b, cache reset
// (refine_plan.h) the grid a refine launch covers, from the stage's margins
inline bool refine_interior(const StageArgs &a, int &rows, int &cols) {
    const Mg m[2] = {a.d[0].own, a.d[1].own};
    return refine_interior(m, a.ndir, rows, cols);
}
void launch_refine_first(const StageArgs &a, hipStream_t st); // the first sweep f64_a -> f64_b (k_refine_first; a.rf_no_prefill)
// a later single sweep f64_a -> f64_b; ev0/ev1 (optional) are recorded right around the light sweep kernel
void launch_refine_sweep(const StageArgs &a, hipStream_t st, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
void launch_refine_apply(const StageArgs &a, hipStream_t st); // k_refine.hip: the update list of launch a.rf_launch into the cache
void launch_refine_rekey(const StageArgs &a, hipStream_t st); // k_refine.hip: both cache ways for the state a.d[].f64_a (k_refine_rekey; a.rf_rekey_far)
// T (2..4) sweeps f64_a -> f64_b in one time-skewed launch (a.rf_launch = launch index, a.skew_rows, a.skew_uw) + the cache-update launch.
// PRECONDITION, the caller's to keep (refine_skew_fits, refine_plan.h; the launcher does not check it): the level is at least 80
// columns wide and every margin lies inside rows 1 .. H - 2 and columns 1 .. W - 2.  The kernel reads rows of 68 columns from the
// flat f64_a, rf_key and rf_ent buffers without clamping (lane 0's column may be as low as -8), and those buffers have no slack.
void launch_refine_skew(const StageArgs &a, int T, hipStream_t st, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr); // k_refine_skew.hip
// T (2..RF_TILE_MAXT) sweeps f64_a -> f64_b in one launch on overlapped tiles (a.rf_launch = launch index) + the cache-update launch
void launch_refine_tile(const StageArgs &a, int T, hipStream_t st); // k_refine_tile.hip

// cloud: returns nothing; *d_npoints (device int64) receives the point count; `flags` = W*H bytes of scratch,
// `blk` = launch_bad_blocks' map (CLOUD_BLOCKS(W,H) bytes)
#define CLOUD_BLOCKS(W, H) ((size_t)(((W) + 31) / 32) * (size_t)(((H) + 31) / 32))
void launch_bad_prefix(const uint8_t *mask, int W, int H, int32_t *prefix, hipStream_t st);
void launch_erode_binary(const int32_t *prefix, int W, int H, int ksize, const int *d_j1, const int *d_j2,
                         uint8_t *dst255, hipStream_t st);
void launch_bad_blocks(const int32_t *prefix, int W, int H, uint8_t *blk, hipStream_t st);
void launch_cloud(const double *disp, const int32_t *bad_prefix, const uint8_t *img, int W, int H, int ksize,
                  const int *d_j1, const int *d_j2, const double *q16_scaled, const double *R,
                  const double *T, Mg own, uint8_t *flags, const uint8_t *blk, int32_t *row_count, int64_t *row_offset,
                  int64_t *d_npoints, double *xyz, uint8_t *bgr, int64_t max_points, hipStream_t st);
void launch_pack_cloud16(const double *xyz, const uint8_t *bgr, int64_t n, void *dst16, hipStream_t st);
void launch_count_masked(const uint8_t *mask, int W, int H, Mg m, unsigned long long *d_count, hipStream_t st);

// Rectify (k_rectify.hip)
void launch_rect_map(const double *ir, double fx, double fy, double u0, double v0, int W, int H, int16_t *map1,
                     uint16_t *map2, hipStream_t st);
void launch_remap(const uint8_t *src, int Ws, int Hs, int C, const int16_t *map1, const uint16_t *map2, int W, int H,
                  uint8_t *dst, hipStream_t st);
// st: ceil(log2(ksize))+1 planes of W*H bytes of scratch
void launch_erode_gray(const uint8_t *src, int W, int H, int ksize, const int *d_j1, const int *d_j2, uint8_t *st,
                       uint8_t *dst, hipStream_t st_);

// cloud filter (k_filter.hip): SOR + radius normals on a device cloud of n float xyz points
// FilterArena (cloud_arena.h; its functions: cloud_grid.hip): grow-only device scratch owned by the context (one hipMalloc per cloud size
// instead of dozens per call)
struct FilterArena;
FilterArena *filter_arena_create();
void filter_arena_destroy(FilterArena *a);
size_t filter_arena_bytes(int64_t n);                      // scratch one filter call needs for n points
int filter_arena_reserve(FilterArena *a, size_t bytes);    // makes room, rewinds the arena
void *filter_arena_alloc(FilterArena *a, size_t bytes);    // caller buffers that live across the call (nullptr: full)
void *filter_arena_host(FilterArena *a);                   // 64 bytes of its pinned host block that no cloud step uses itself: free for the caller (after a reserve)
// The cloud as the depth map it is (rsm_filter_last_cloud): which pixels of the top level's margin box emitted a point (k_cloud's
// flags + per-row offsets: point index = compaction order), the fp64 points, and the geometry that bounds how far a point outside
// a pixel window can be (k_filter_win.hip: k_sor_window; win_bound.h).  R_final must be a rotation (the caller checks).
// What the passes behind the tile pass did (rsm_filter_last_passes): every pass that ran in the wave or the workgroup form -- the 24- / 40-pixel
// passes when "filter_list" puts them there, then 80, 160, ... -- and what reached the searches behind them.
#define FILTER_MAX_PASSES 16
struct FilterPasses {
    int n = 0;                                    // passes recorded
    int radius[FILTER_MAX_PASSES] = {};           // window radius in pixels
    int entered[FILTER_MAX_PASSES] = {};          // queries the pass was given
    int decided[FILTER_MAX_PASSES] = {};          // queries it decided
    int workgroup[FILTER_MAX_PASSES] = {};        // 1: four waves per query (k_sor_window_wg), 0: a wave per query (k_sor_window_wave)
    int ladder_in = 0;                            // queries handed to the grid ladder (0: it did not run)
    int whole_in = 0, whole_over_lattice = 0;     // queries handed to the whole-cloud search; whether it read the lattice copy as its point array
};
struct FilterLattice {
    const uint8_t *flags;
    const int64_t *row_offset;
    int W, XL, XR, YL, YR;
    const double *xyz64;
    double qz;          // Q[2][3] * scale (CStereoMatching.cpp:698)
    double R[9], T[3];  // R_final, T_final (host copies)
    int radius;         // window radius in pixels: 7, 12, 16, 20 or 24; 0 = chosen from a sparse probe (7 / 12 / 16, or no window pass)
    int *radius_out;    // optional: the radius used (0: the probe found no window worth its pass)
    int list_pass;      // 1: what the tile pass leaves over gets a 24-pixel window a thread each before the grid ladder
    int *undecided_out; // optional: queries the window passes left to the grid ladder
    int *tile_left_out; // optional: queries the tile pass alone left over
    int wg_max;         // the wave passes take four waves per query (k_sor_window_wg) while at most this many queries are left (default 2048)
    int normals_wmax;   // the normals' radius search on the lattice copy while no point needs a window wider than this (0: always on a grid of radius-cells)
    int *normals_out;   // optional, 2 ints: the window the normals used (0: the grid), the widest window a point needed
    FilterPasses *passes_out; // optional: what the wave passes, the ladder and the whole-cloud search were given
};
// The radius outlier pass between the outlier removal and the normals (k_filter_outrem.hip; rsm_filter_set_outrem, rsm_filter_last_outrem):
// a survivor of the first pass stays iff more than min_neighbors finite survivors (itself included) lie within radius of it.
struct FilterOutrem {
    bool on = false;          // in
    int min_neighbors = 0;    // in: >= 0
    double radius = 0.0;      // in: positive, finite, with a positive finite float32 square and a positive float32 value (the setter checks)
    int64_t points_in = -1;   // out: the first pass's survivors (-1: the pass was off)
    int64_t removed = 0;      // out: of them, removed here
    int64_t nonfinite = 0;    // out: non-finite points among the removed
    int window = 0;           // out: the pixel window the count ran over on the lattice copy (0: the grid of radius-cells)
};
// The k-nearest grid ladder's route (option "filter_ladder_h", rsm_filter_last_grid): which levels decide a query, never its result --
// and the radius outlier pass's setting and report, which travel with it through every filter entry.
struct FilterRoute {
    float h0 = 0.0f;        // in: > 0 pins the first level's search radius (0: from the sample's extent, as without a route)
    float h = 0.0f;         // out: the first level's search radius (0: no level ran)
    float origin[3] = {};   // out: its grid origin (world x, y, z)
    int cells[3] = {};      // out: its cells per world axis
    int levels = 0;         // out: levels run
    int kind0 = -1;         // out: the first level's cell table kind (-1: no level ran)
    int kinds = 0;          // out: bit t set when a level searched with table kind t (k_sor_knn<t>)
    FilterOutrem outrem;    // in: the radius outlier pass (off by default); out: what it did
};
size_t cloud_lattice_bytes(int XL, int XR, int YL, int YR); // k_filter_win.hip
int filter_cloud_device(FilterArena *a, const float *d_xyz, int64_t n, int mean_k, double std_mul, double normal_radius,
                        const float cam_center[3], int32_t *d_kept_index, float *d_fxyz, float4 *d_normals, int64_t *n_kept,
                        double stats[4], hipStream_t st, const FilterLattice *pre = nullptr, FilterRoute *route = nullptr);
// the radius outlier pass's count alone, on the grid route (rsm_stage_radius_count): d_count[i] = min(count(p_i), cap) over the whole cloud
// as S (k_filter_outrem.hip's definition); A as above
int radius_count_device(FilterArena *a, const float *d_xyz, int64_t n, double radius, int cap, int32_t *d_count, hipStream_t st);
void launch_f64_to_f32x3(const double *src, int64_t n, float *dst, hipStream_t st);
void launch_pack_filtered16(const double *xyz, const uint8_t *bgr, const int32_t *kept, int64_t m, void *dst16, hipStream_t st);

// moving-least-squares smoothing (k_mls.hip; CCloudOptimization::run, CCloudOptimization.cpp:348-389) of n float xyz points, on the
// filter's arena: d_ref (optional) n float4 normals to agree with; outputs in input order, *n_out of them (one host round trip)
size_t mls_arena_bytes(int64_t n); // scratch one call needs for n points (callers add their own buffers)
int mls_cloud_device(FilterArena *a, const float *d_xyz, int64_t n, const float4 *d_ref, double radius, int order, float *d_oxyz, float *d_onrm,
                     int32_t *d_oidx, int64_t *n_out, hipStream_t st);
void launch_point16_xyz(const void *rec, int64_t n, float *xyz, hipStream_t st); // rsm_point16 records -> n x 3 float

// multi-view duplicate deletion (k_dedup.hip; CCloudOptimization::run's isdelete branch, CCloudOptimization.cpp:152-346): one pair as the
// kernels see it -- R / T of both views as float (cv2eigen of P's columns), CamCenter, the left bound, the images on the device, and
// the first key of the pair's buckets
struct DedupPair {
    float R0[9], T0[3], R1[9], T1[3], C[3];
    int XL, YL, bw, bh, W, H;
    unsigned long long base;
    const uint8_t *img0, *img1, *m0, *m1;
};
struct rsm_dedup_view;
int dedup_views_ok(const rsm_dedup_view *v, int n_pairs); // bounds inside their images, 2 px from the edge (empty bounds pass)
size_t dedup_arena_bytes(const rsm_dedup_view *v, int n_pairs, int64_t n); // scratch one call needs (images included; callers add theirs)
// n points (float x, y, z at d_pts[stride * j]) with float4 normals -> d_index (capacity n) = indicesptr, *n_out of them; stats = s1, s2,
// count0, buckets visited.  Uploads the views' host images into the arena; one host round trip after the sort, one at the end.
int dedup_cloud_device(FilterArena *a, const float *d_pts, int stride, const float4 *d_nrm, int64_t n, const rsm_dedup_view *v, int n_pairs,
                       int32_t *d_index, int64_t *n_out, int64_t stats[4], hipStream_t st);
// the kept points as rsm_point16 records and their float4 normals (either output may be NULL), what rsm_mls_cloud_device reads
void launch_dedup_gather(const void *d_rec, const float *d_nrm, const int32_t *d_idx, int64_t m, void *d_orec, float *d_onrm, hipStream_t st);

// dense-grid Poisson surface and trim (k_poisson.hip).  Device buffers: n float xyz (stride 3), n float4 normals.
struct PoissonMesh { // a library-owned result: nv float xyz, nf int32 x 3
    float *d_v = nullptr;
    int32_t *d_f = nullptr;
    int64_t nv = 0, nf = 0;
};
void poisson_mesh_free(PoissonMesh *m);
// grid = {origin x, y, z, h} (h = 0: no valid sample or all points equal), counts = {valid, not valid}; d_nrm4 = NULL: a finite point is valid
int poisson_grid_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, double scale, double grid[4], int64_t counts[2], hipStream_t st);
// splat + right-hand side: b as float (the solver's) and / or as double (exact from the fixed-point sums), occ = N^3 bytes
int poisson_rhs_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, const double grid[4], float *d_b32, double *d_b64, uint8_t *d_occ,
                       hipStream_t st);
// RSM_OK, RSM_W_NOT_CONVERGED or an error; history (optional, max_cycles doubles) = the residual after each cycle
int poisson_solve_device(const float *d_b, int depth, double rel_residual, int max_cycles, float *d_chi, double *residual, int *cycles, double *history,
                         hipStream_t st);
int poisson_iso_device(const float *d_xyz, const float *d_nrm4, int64_t n, int64_t n_valid, const float *d_chi, int depth, const double grid[4], double *iso,
                       hipStream_t st);
// the two halves of the iso-value, which the density-adaptive form (k_poisson_density.hip) weighs between them.  Both enqueue only.
// chi's trilinear interpolation at the n samples (0 at the samples that take no part) -> d_val, n doubles
void poisson_chi_at_samples(const float *d_xyz, const float *d_nrm4, int64_t n, const float *d_chi, int depth, const double grid[4], double *d_val, hipStream_t st);
// the sum of n doubles in f7's fixed tree (it depends on n only) -> *d_sum; d_part = POISSON_SUM_PARTIALS doubles of scratch
#define POISSON_SUM_PARTIALS 1024
void poisson_tree_sum(const double *d_v, int64_t n, double *d_part, double *d_sum, hipStream_t st);
// d_occ may be NULL with trim_cells = 0; untrimmed = {vertices, faces} before the trim
int poisson_extract_device(const float *d_chi, int depth, double iso, const double grid[4], const uint8_t *d_occ, int trim_cells, PoissonMesh *out,
                           int64_t untrimmed[2], hipStream_t st);

// the density-adaptive form of the splat and the right-hand side (k_poisson_density.hip), on a box with grid[3] > 0.
// d_depth_in (n doubles, may be NULL): each sample's depth from the caller instead of from its density.  d_rho / d_w / d_d: n doubles each,
// 0 at the samples that take no part.  sample_stats = {the least d_s, samples with d_s < depth, sum of w_s (f7's fixed tree)}
int poisson_density_rhs_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, const double grid[4], int kernel_depth, double samples_per_node,
                               const double *d_depth_in, float *d_b32, double *d_b64, uint8_t *d_occ, double *d_rho, double *d_w, double *d_d,
                               double sample_stats[3], hipStream_t st);
// ... in its parts, for the banded call with this splat (k_poisson_band_density.hip; f17), which keeps the finest level on its bricks:
// items 2 and 3 alone: d_rho, d_w, d_d and sample_stats as above
int poisson_density_samples_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, const double grid[4], int kernel_depth, double samples_per_node,
                                   const double *d_depth_in, double *d_rho, double *d_w, double *d_d, double sample_stats[3], hipStream_t st);
// the 64-bit words of a level buffer whose top level is `top`
size_t poisson_density_level_words(int top);
// items 4 and 5 on the levels 3..top (top <= depth) of the grid whose finest level is `depth` with step grid[3]: d_d is clamped to depth, what
// falls on a level above top is left out, the scales are 8^(L - depth).  d_V: poisson_density_level_words(top) words, zeroed here; *d_U_top:
// the top level's three components in it, fp64.  d_occ (2^(3 depth) bytes) may be NULL.  Enqueues only.
int poisson_density_levels_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, int top, const double grid[4], const double *d_w, const double *d_d,
                                  unsigned long long *d_V, uint8_t *d_occ, const double **d_U_top, hipStream_t st);
// item 6 of a field d_U of three components on 2^depth nodes per axis.  Enqueues only.
void poisson_density_rhs_of_field(const double *d_U, int depth, float *d_b32, double *d_b64, hipStream_t st);
// sum w_s val_s / sum_w in f7's tree; d_val (n doubles) is overwritten
int poisson_weighted_mean_device(double *d_val, const double *d_w, int64_t n, double sum_w, double *mean, hipStream_t st);
// iso = sum w_s chi(p_s) / sum_w over the samples (sum_w = sample_stats[2])
int poisson_iso_weighted_device(const float *d_xyz, const float *d_nrm4, int64_t n, const double *d_w, double sum_w, const float *d_chi, int depth,
                                const double grid[4], double *iso, hipStream_t st);

// the banded finest level on top of the dense solve (k_poisson_band.hip).  A band: the active bricks (8^3 nodes each) of the
// grid of 2^depth nodes per axis in ascending linear index; fields are brick-major, n_active * 512 elements.
struct PoissonBand {
    int depth = 0;
    int64_t n_active = 0, n_occupied = 0;
    int32_t *d_slot = nullptr;   // (2^(depth-3))^3: brick -> slot, -1 inactive
    int32_t *d_active = nullptr; // n_active: slot -> brick
    int32_t *d_nbr = nullptr;    // n_active x 27: the slots around a slot (-1 inactive, -2 outside the grid)
};
void poisson_band_free(PoissonBand *b);
// the bricks within band_bricks of a brick that holds a valid sample's cell.  More than max_bricks of them: RSM_OK with n_active set and no
// tables (the caller refuses by name)
int poisson_band_bricks_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, const double grid[4], int band_bricks, int64_t max_bricks,
                               PoissonBand *out, hipStream_t st);
// ... from a caller's list on the host (ascending, each in range: the caller checks)
int poisson_band_of_list_device(const int32_t *h_bricks, int64_t n_bricks, int depth, PoissonBand *out, hipStream_t st);
// f7's splat and right-hand side on the band: d_b32 / d_b64 (either may be NULL) and d_occ (per fine cell), brick-major
int poisson_band_rhs_device(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, const double grid[4], float *d_b32, double *d_b64,
                            uint8_t *d_occ, hipStream_t st);
// g = (float)(1/4 of the trilinear prolongation of d_chi_c, the dense field of depth - 1)
int poisson_band_guess_device(const PoissonBand &band, const float *d_chi_c, float *d_g, hipStream_t st);
// d_chi: the guess on entry, the best field on return.  d_chi_c (may be NULL: 0) gives the guess at the inactive neighbours of the band.
// residual0: before the first iteration; history (optional): max_iterations doubles.  RSM_OK / RSM_W_NOT_CONVERGED / an error
int poisson_band_solve_device(const PoissonBand &band, const float *d_b, const float *d_chi_c, double rel_residual, int max_iterations, float *d_chi,
                              double *residual0, double *residual, int *iterations, double *history, hipStream_t st);
int poisson_band_iso_device(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, int64_t n_valid, const float *d_chi,
                            const double grid[4], double *iso, hipStream_t st);
int poisson_band_extract_device(const PoissonBand &band, const float *d_chi, double iso, const double grid[4], const uint8_t *d_occ, int trim_cells,
                                PoissonMesh *out, int64_t untrimmed[2], hipStream_t st);
// chi's trilinear interpolation at the n samples on the band (0 at the samples that take no part) -> d_val, n doubles.  Enqueues only.
void poisson_band_chi_at_samples(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, const float *d_chi, const double grid[4], double *d_val,
                                 hipStream_t st);

// the banded finest level with the density-adaptive splat (k_poisson_band_density.hip).  d_w, d_d: poisson_density_samples_device's
// at the finest depth.  d_levels: poisson_density_level_words(band.depth - 1) words of scratch (the levels 3..depth - 1, dense).  d_b32 / d_b64
// (either may be NULL) and d_occ (per fine cell), brick-major
int poisson_band_density_rhs_device(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, const double grid[4], const double *d_w,
                                    const double *d_d, unsigned long long *d_levels, float *d_b32, double *d_b64, uint8_t *d_occ, hipStream_t st);
// iso = sum w_s chi(p_s) / sum_w with chi on the band
int poisson_band_iso_weighted_device(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, const double *d_w, double sum_w, const float *d_chi,
                                     const double grid[4], double *iso, hipStream_t st);

// smoothing and clean-up of a triangle mesh (k_meshclean.hip).  Device buffers: nv float xyz, nf int32 x 3.  RSM_E_INVALID
// comes with *invalid = 1 (a face index outside [0, nv)) or 2 (a coordinate that is not finite); parameters are the caller's to check.
struct rsm_mesh_clean_params;
// d_out may not alias d_v; *n_border = the endpoints of incidence-1 edges
int mesh_smooth_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, int steps, int cotangent, int boundary, float *d_out, int64_t *n_border,
                       int *invalid, hipStream_t st);
// d_label[f] = the lowest face index of f's component (-1: a face with a repeated index)
int mesh_components_device(const int32_t *d_f, int64_t nv, int64_t nf, int32_t *d_label, int64_t *n_components, int *invalid, hipStream_t st);
// the result replaces *out, which may own d_v / d_f (it is freed after the last read); stats: RSM_MESH_CLEAN_STATS doubles, may be NULL
int mesh_clean_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_mesh_clean_params *p, PoissonMesh *out, double *stats, int *invalid,
                      hipStream_t st);

// the closing of the surface's small holes (k_meshclose.hip).  Device buffers: nv float xyz, nf int32 x 3; *invalid as
// mesh_clean_device's; parameters are the caller's to check.
struct rsm_mesh_close_params;
// per entry 3 f + j (3 nf int32 each): d_label = the lowest entry of its border component (-1: no border entry), d_size = L for a loop's
// entries, 0 for an open component's, -1 otherwise
int mesh_border_loops_device(const int32_t *d_f, int64_t nv, int64_t nf, int32_t *d_label, int32_t *d_size, int64_t *n_components, int *invalid, hipStream_t st);
// one ring of L (3 .. RSM_MESH_CLOSE_MAX_HOLE) finite points, d_mask = L x L bytes of forbidden pairs or NULL -> *weight = W(0, L-1),
// d_tri (L - 2 triangles of ring positions), *n_tri = L - 2, or +inf and 0
int hole_triangulate_device(const float *d_ring, int L, const uint8_t *d_mask, double *weight, int32_t *d_tri, int *n_tri, hipStream_t st);
// the whole call; the result replaces *out, which may own d_v / d_f; stats: RSM_MESH_CLOSE_STATS doubles, may be NULL
int mesh_close_holes_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_mesh_close_params *p, PoissonMesh *out, double *stats,
                            int *invalid, hipStream_t st);

// the decimation of the final mesh (k_meshdecimate.hip).  Device buffers: nv float xyz, nf int32 x 3, quadrics nv x 10
// double; *invalid as mesh_clean_device's; parameters are the caller's to check.
struct rsm_mesh_decimate_params;
int mesh_quadrics_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, double boundary_weight, double *d_q, int *invalid, hipStream_t st);
// per unique edge in key order (room for 3 nf each): key, multiplicity, cost (+inf: no candidate), reject code, position
int mesh_collapse_costs_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const double *d_q, const rsm_mesh_decimate_params *p, uint64_t *d_key,
                               int32_t *d_mult, double *d_cost, int32_t *d_reject, float *d_pos, int64_t *n_edges, int *invalid, hipStream_t st);
// one round: d_v and d_q are updated in place, the faces go to d_fout (room for nf), the selected keys in priority order to d_sel (room for 3 nf)
int mesh_collapse_round_device(float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, double *d_q, const rsm_mesh_decimate_params *p, int64_t need, int32_t *d_fout,
                               int64_t *nf_out, uint64_t *d_sel, int64_t *n_selected, int64_t *n_kept, int *invalid, hipStream_t st);
// the whole call; the result replaces *out, which may own d_v / d_f; stats: RSM_MESH_DECIMATE_STATS doubles, may be NULL
int mesh_decimate_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_mesh_decimate_params *p, PoissonMesh *out, double *stats,
                         int *invalid, hipStream_t st);

// the Loop subdivision of the final mesh (k_meshsubdivide.hip).  Device buffers: nv float xyz, nf int32 x 3; *invalid as
// mesh_clean_device's, or MESH_INVALID_TOO_LARGE + it: iteration it (from 0) would leave more than INT32_MAX vertices or 3 nf >= 2^31
// (csrc/subdivide_limits.h); parameters are the caller's to check.
#define MESH_INVALID_TOO_LARGE 16
struct rsm_mesh_subdivide_params;
// one iteration's decisions.  Per unique edge in key order (room for 3 nf each): key, multiplicity, whether it splits, the odd point (zeros
// where it does not); per vertex: the class (0 interior, 1 border, 2 locked) and the even point; *thr_used: the threshold of the call
int mesh_subdivide_edges_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_mesh_subdivide_params *p, uint64_t *d_key, int32_t *d_mult,
                                int32_t *d_split, float *d_odd, int64_t *n_edges, int32_t *d_class, float *d_even, double *thr_used, int *invalid, hipStream_t st);
// the whole call; the result replaces *out, which may own d_v / d_f, and only at the very end: a failed call leaves *out as it was.
// stats: RSM_MESH_SUBDIVIDE_STATS doubles, may be NULL
int mesh_subdivide_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_mesh_subdivide_params *p, PoissonMesh *out, double *stats,
                          int *invalid, hipStream_t st);

// the density trim of the surface (k_meshtrim.hip).  Device buffers: n float xyz samples with float4 normals (d_sn4 may be
// NULL: a finite point is a valid sample), nv float xyz, nf int32 x 3.  Parameters are the caller's to check; each call validates the
// mesh it is given, and RSM_E_INVALID comes with *invalid as mesh_clean_device's.
struct rsm_mesh_trim_params;
// rho (may be NULL) and value at the vertices; counts = {valid, not valid} samples, *hk = the density grid's step (0: every value is 0)
int mesh_density_device(const float *d_sx, const float *d_sn4, int64_t n, int depth, double scale, int kernel_depth, double samples_per_node, const float *d_v,
                        int64_t nv, double *d_rho, double *d_val, int64_t counts[2], double *hk, int *invalid, hipStream_t st);
// nv values after `steps` steps over the mesh's incidences; d_out may not alias d_in
int mesh_value_smooth_device(const int32_t *d_f, int64_t nv, int64_t nf, const double *d_in, int steps, double *d_out, int *invalid, hipStream_t st);
// split, island rule and compaction of a mesh by nv values; the result replaces *out, which may own d_v / d_f.  d_src / d_side /
// d_label (each 3 nf int32, may be NULL): per output face its source face, its side before the island rule, its component's lowest triangle
int mesh_split_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const double *d_val, double trim, double island_ratio, PoissonMesh *out,
                      int32_t *d_src, int32_t *d_side, int32_t *d_label, double *stats, int *invalid, hipStream_t st);
// the whole call
int mesh_trim_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const float *d_sx, const float *d_sn4, int64_t n, const rsm_mesh_trim_params *p,
                     PoissonMesh *out, double *stats, int *invalid, hipStream_t st);

// colours of a mesh from the rig's views (k_meshcolor.hip).  Device buffers: nv float xyz, nf int32 x 3, d_rgb nv x 3 bytes,
// d_best nv int32 (may be NULL); the views' images are host pointers and are uploaded here.  RSM_E_INVALID comes with *invalid = 1 (a face
// index outside [0, nv)), 2 (a coordinate that is not finite) or 3 (a singular P); parameters and views are the caller's to check.
// big_box: a (face, view) box of more pixels is strided by a block instead of walked by one thread.
struct rsm_mesh_color_params;
int mesh_color_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *p,
                      long long big_box, uint8_t *d_rgb, int32_t *d_best, double *stats, int *invalid, hipStream_t st);
// one view's depth buffer: W x H uint32, the largest float32 bit pattern of the inverse depth drawn at each pixel centre, 0 where nothing is
int mesh_depth_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const double P12[12], int W, int H, long long big_box, uint32_t *d_wbuf,
                      int *invalid, hipStream_t st);
// texture_color (CCloudOptimization.cpp:400-421) of n points against a BGR image on the device
int texture_color_device(const float *d_xyz, int64_t n, const double P12[12], const uint8_t *d_img, int W, int H, uint8_t *d_rgb, hipStream_t st);

// the views' exposure seams levelled in those colours (k_meshstitch.hip).  mesh_stitch_device: mesh_color_device's
// arguments (mode 0; d_best may be NULL) and the stitch parameters, d_rgb = the levelled bytes, stats = RSM_MESH_STITCH_STATS doubles (may
// be NULL); *invalid as there, or 4 (the reduction needs more than RSM_MESH_STITCH_MAX_ITERATIONS steps).  Parameters, views and V <= 64
// are the caller's to check.
struct rsm_mesh_stitch_params;
int mesh_stitch_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *cp,
                       const rsm_mesh_stitch_params *sp, long long big_box, uint8_t *d_rgb, int32_t *d_best, double *stats, int *invalid, hipStream_t st);
// the least k with T_k(sigma) >= 1 / reduction by the recurrence; -1: more than RSM_MESH_STITCH_MAX_ITERATIONS
int mesh_stitch_steps(double lambda, unsigned long long dmax, double reduction);
// the stages: d_vis nv uint64 (bit v = view v sees the vertex); d_best's values lie in -1 .. V - 1 (the caller's to check)
int mesh_visibility_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *p,
                           long long big_box, unsigned long long *d_vis, int *invalid, hipStream_t st);
int mesh_stitch_rhs_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_dedup_view *views, int n_pairs, const uint8_t *d_rgb,
                           const int32_t *d_best, const unsigned long long *d_vis, int seam_gradient, double *d_G, int32_t *d_deg, int64_t counts[5], int *invalid,
                           hipStream_t st);
int mesh_stitch_solve_device(const int32_t *d_f, int64_t nv, int64_t nf, const int32_t *d_best, const uint8_t *d_rgb, const double *d_G, double lambda,
                             int iterations, double *d_x, double *rel_residual, int *invalid, hipStream_t st);

// the vertices no view sees filled from the colours around them (k_meshfill.hip).  Device buffers: d_rgb nv x 3 bytes in
// and out, d_best nv int32, d_level nv int32 out (-1 unreached; may be NULL in mesh_fill_device); batch = the rounds between two read-backs;
// stats = RSM_MESH_FILL_STATS doubles (may be NULL).  RSM_E_INVALID comes with *invalid = 1 (a face index outside [0, nv)) or 4 (the
// reduction needs more than RSM_MESH_FILL_MAX_ITERATIONS steps); the parameters are the caller's to check.
struct rsm_mesh_fill_params;
int mesh_fill_device(const int32_t *d_f, int64_t nv, int64_t nf, const int32_t *d_best, uint8_t *d_rgb, int32_t *d_level, const rsm_mesh_fill_params *p, int batch,
                     double *stats, int *invalid, hipStream_t st);
// the least k with T_k(sigma) >= 1 / reduction at lmin = 1 / (2 (L + 1))^2; -1: more than RSM_MESH_FILL_MAX_ITERATIONS
int mesh_fill_steps(int L, double reduction);
// the stages: the front alone -> d_x nv x 3 doubles, d_level, *L; `iterations` steps from a caller's d_x (in and out), d_level and L
int mesh_fill_front_device(const int32_t *d_f, int64_t nv, int64_t nf, const int32_t *d_best, const uint8_t *d_rgb, int max_rounds, int batch, double *d_x,
                           int32_t *d_level, int *L, int *invalid, hipStream_t st);
int mesh_fill_solve_device(const int32_t *d_f, int64_t nv, int64_t nf, const int32_t *d_level, int L, int iterations, double *d_x, int *invalid, hipStream_t st);
