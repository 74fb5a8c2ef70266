// rsm_stages.hip -- the parity and benchmark entry points of the matcher and of Rectify: one stage, host buffers in and out,
// one direction (include/rsm.h: rsm_stage_*, rsm_bench_ncc).  rsm_stage_refine lives beside refine_sweeps in rsm_refine.hip.
#include "rectify_host.h"
#include "rsm_ctx.h"

#include <algorithm>
#include <math.h>
#include <string.h>

extern "C" int rsm_stage_find_margin(rsm_ctx *c, const uint8_t *mask, int W, int H, int r, rsm_boundary *m) {
    if (!stage_ok(c, W, H) || !mask || !m) return RSM_E_INVALID;
    Tmp t(c);
    uint8_t *dm = t.up(mask, (size_t)W * H);
    int *d4 = t.alloc<int>(4);
    if (!t.ok) return finish(c, t);
    launch_find_margin(dm, W, H, r, d4, c->stream);
    int h[4];
    t.down(h, d4, 4);
    *m = to_boundary(Mg{h[2], h[3], h[0], h[1]});
    return finish(c, t);
}

extern "C" int rsm_stage_pyr_down(rsm_ctx *c, const uint8_t *src, int W, int H, int ch, uint8_t *dst) {
    if (!stage_ok(c, W, H) || !src || !dst || (ch != 1 && ch != 3)) return RSM_E_INVALID;
    Tmp t(c);
    const size_t nd = (size_t)((W + 1) / 2) * ((H + 1) / 2) * ch;
    uint8_t *ds = t.up(src, (size_t)W * H * ch);
    uint8_t *dd = t.alloc<uint8_t>(nd);
    if (!t.ok) return finish(c, t);
    launch_pyr_down(ds, W, H, ch, dd, c->stream);
    t.down(dst, dd, nd);
    return finish(c, t);
}

extern "C" int rsm_stage_erode_ellipse(rsm_ctx *c, const uint8_t *mask, int W, int H, int ksize, uint8_t *dst) {
    if (!stage_ok(c, W, H) || !mask || !dst || ksize < 1 || ksize > 4096) return RSM_E_INVALID;
    Tmp t(c);
    std::vector<int> j1, j2;
    ellipse_spans(ksize, j1, j2);
    uint8_t *dm = t.up(mask, (size_t)W * H);
    int *d1 = t.up(j1.data(), (size_t)ksize), *d2 = t.up(j2.data(), (size_t)ksize);
    int32_t *pre = t.alloc<int32_t>((size_t)(W + 1) * H);
    uint8_t *dd = t.alloc<uint8_t>((size_t)W * H);
    if (!t.ok) return finish(c, t);
    launch_bad_prefix(dm, W, H, pre, c->stream);
    launch_erode_binary(pre, W, H, ksize, d1, d2, dd, c->stream);
    t.down(dst, dd, (size_t)W * H);
    return finish(c, t);
}

extern "C" int rsm_stage_box_sums(rsm_ctx *c, const uint8_t *img_bgr, int W, int H, int r, int32_t *S1, int32_t *S2) {
    if (!stage_ok(c, W, H) || !img_bgr || !S1 || !S2 || r < 1 || r > 15) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    uint8_t *di = t.up(img_bgr, px * 3);
    uint32_t *i4 = t.alloc<uint32_t>(px);
    int32_t *d1 = t.alloc<int32_t>(px), *d2 = t.alloc<int32_t>(px);
    int32_t *t1 = t.alloc<int32_t>(px), *t2 = t.alloc<int32_t>(px);
    if (!t.ok) return finish(c, t);
    launch_bgr_to_bgrx(di, W, H, i4, c->stream); // the sequence of setup_match below
    launch_box_sums(i4, W, H, r, t1, t2, d1, d2, c->stream);
    t.down(S1, (const int32_t *)d1, px);
    t.down(S2, (const int32_t *)d2, px);
    return finish(c, t);
}

namespace {
// uploads the images/masks of one direction and builds the window-sum tables
struct MatchBufs {
    uint8_t *io, *it, *mo, *mt;
    uint32_t *i4o, *i4t;
    uint32_t *wl; // wide-pixel worklist + counter of the NCC kernels
    int32_t *wc;
    uint32_t *tl; // tie list + counters (k_ncc_exact)
    int32_t *tc;
    int32_t *wr;  // wide pixels per row
    int32_t *S1o, *S2o, *S1t, *S2t;
};
bool setup_match(rsm_ctx *c, Tmp &t, const uint8_t *img_own, const uint8_t *img_oth, const uint8_t *mask_own,
                 const uint8_t *mask_oth, int W, int H, int r, MatchBufs &b) {
    const size_t px = (size_t)W * H;
    b.io = t.up(img_own, px * 3);
    b.it = t.up(img_oth, px * 3);
    b.mo = t.up(mask_own, px);
    b.mt = t.up(mask_oth, px);
    b.wl = t.alloc<uint32_t>(std::max(px + 64, SETB_SCRATCH(W))); // NCC worklist / SetBoundary scratch
    b.wc = t.alloc<int32_t>(16 + 2 * (size_t)H);
    if (b.wc) (void)hipMemsetAsync(b.wc, 0, sizeof(int), c->stream); // wide-pixel counter of the NCC launch
    b.tl = t.alloc<uint32_t>(px + 64);
    b.tc = t.alloc<int32_t>(2);
    if (b.tc) (void)hipMemsetAsync(b.tc, 0, 2 * sizeof(int), c->stream);
    b.wr = t.alloc<int32_t>(NCC_WROW_INTS((size_t)H));
    if (b.wr) (void)hipMemsetAsync(b.wr, 0, sizeof(int32_t) * NCC_WROW_INTS((size_t)H), c->stream);
    b.i4o = t.alloc<uint32_t>(px);
    b.i4t = t.alloc<uint32_t>(px);
    b.S1o = t.alloc<int32_t>(px);
    b.S2o = t.alloc<int32_t>(px);
    b.S1t = t.alloc<int32_t>(px);
    b.S2t = t.alloc<int32_t>(px);
    int32_t *t1 = t.alloc<int32_t>(px), *t2 = t.alloc<int32_t>(px);
    if (!t.ok) return false;
    launch_bgr_to_bgrx(b.io, W, H, b.i4o, c->stream);
    launch_bgr_to_bgrx(b.it, W, H, b.i4t, c->stream);
    launch_box_sums(b.i4o, W, H, r, t1, t2, b.S1o, b.S2o, c->stream);
    launch_box_sums(b.i4t, W, H, r, t1, t2, b.S1t, b.S2t, c->stream);
    return true;
}
void bind_match(StageArgs &a, const MatchBufs &b) {
    a.rf_list = b.wl;
    a.ncc_cnt = b.wc;
    a.tie_list = b.tl;
    a.tie_cnt = b.tc;
    a.wrow = b.wr;
    DirArgs &d = a.d[0];
    d.img_own = b.io;
    d.img_oth = b.it;
    d.img4_own = b.i4o;
    d.img4_oth = b.i4t;
    d.mask_own = b.mo;
    d.mask_oth = b.mt;
    d.S1_own = b.S1o;
    d.S2_own = b.S2o;
    d.S1_oth = b.S1t;
    d.S2_oth = b.S2t;
}
} // namespace

extern "C" int rsm_stage_initial_match(rsm_ctx *c, const uint8_t *img_own, const uint8_t *img_oth,
                                       const uint8_t *mask_own, const uint8_t *mask_oth, int W, int H, int r,
                                       int offset, const rsm_boundary *own, const rsm_boundary *oth,
                                       const double *parent, int Wp, int Hp, int16_t *disp) {
    if (!stage_ok(c, W, H) || !img_own || !img_oth || !mask_own || !mask_oth || !own || !oth || !disp) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    MatchBufs b{};
    if (!setup_match(c, t, img_own, img_oth, mask_own, mask_oth, W, H, r, b)) return finish(c, t);
    StageArgs a = one_dir(c, W, H, r, own, oth);
    bind_match(a, b);
    a.offset = offset;
    a.Wp = Wp;
    a.Hp = Hp;
    int16_t *dd = t.alloc<int16_t>(px);
    a.d[0].BL = t.alloc<int16_t>(px);
    a.d[0].BR = t.alloc<int16_t>(px);
    if (!t.ok) return finish(c, t);
    launch_fill_i16(dd, px, (int16_t)NOMATCH, c->stream);
    a.d[0].d16_in = a.d[0].d16_out = dd;
    if (!parent) {
        launch_ncc_argmax(a, 0, c->stream);
    } else {
        double *dp = t.up(parent, (size_t)Wp * Hp);
        int32_t *nv = t.alloc<int32_t>((size_t)Wp * Hp);
        if (!t.ok) return finish(c, t);
        a.d[0].parent = dp;
        a.d[0].parent_nv = nv;
        launch_next_valid(dp, Wp, Hp, nv, c->stream);
        launch_hl_interval(a, c->stream);
        launch_ncc_argmax(a, 1, c->stream);
    }
    t.down(disp, dd, px);
    // the routing witness, copied before the scratch is freed
    c->ncc_wit_H = 0;
    std::vector<int32_t> wr(NCC_WROW_INTS((size_t)H));
    int32_t cnt = 0, ties = 0;
    t.down(wr.data(), b.wr, wr.size());
    t.down(&cnt, b.wc, 1);
    t.down(&ties, b.tc, 1);
    const int s = finish(c, t);
    if (s == RSM_OK) {
        c->ncc_wit_wrow.swap(wr);
        c->ncc_wit_H = H;
        c->ncc_wit_cnt = cnt;
        c->ncc_wit_ties = ties;
    }
    return s;
}

extern "C" int rsm_stage_last_ncc_routes(rsm_ctx *c, int H, int32_t *wide, int32_t *mid, int32_t *widest, int32_t *route,
                                         int64_t *worklist, int64_t *ties) {
    if (!c || !wide || !mid || !widest || !route || !worklist || !ties) return RSM_E_INVALID;
    if (c->ncc_wit_H == 0) return set_err(c, RSM_E_STATE, "no rsm_stage_initial_match has run on this context");
    if (H != c->ncc_wit_H) return set_err(c, RSM_E_INVALID, "H %d: the last initial match had %d rows", H, c->ncc_wit_H);
    const int32_t *w = c->ncc_wit_wrow.data();
    for (int y = 0; y < H; y++) {
        wide[y] = w[y];
        mid[y] = w[NCC_WROW_MID(H) + y];
        widest[y] = w[NCC_WROW_MAX(H) + y];
        route[y] = w[y] > 0 ? 1 : 0;
    }
    for (int which = 0; which < 2; which++) { // list 0: k_ncc_rowgemm, list 1: k_ncc_slide ([0] = count, then the rows)
        const int32_t *l = w + NCC_WROW_LIST(H, which);
        const int n = std::min(std::max(l[0], 0), H);
        for (int i = 0; i < n; i++) {
            const int y = l[1 + i];
            if (y < 0 || y >= H) return set_err(c, RSM_E_STATE, "row list %d holds row %d of %d", which, y, H);
            route[y] = route[y] >= 2 ? -1 : 2 + which; // -1: a row listed twice
        }
    }
    *worklist = c->ncc_wit_cnt;
    *ties = c->ncc_wit_ties;
    return RSM_OK;
}

extern "C" int rsm_stage_smooth(rsm_ctx *c, int16_t *disp, int W, int H, const rsm_boundary *own) {
    if (!stage_ok(c, W, H) || !disp || !own) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    StageArgs a = one_dir(c, W, H, 0, own, nullptr);
    a.d[0].d16_in = t.up(disp, px);
    a.d[0].d16_out = t.alloc<int16_t>(px);
    if (!t.ok) return finish(c, t);
    launch_smooth(a, c->stream);
    t.down(disp, a.d[0].d16_out, px);
    return finish(c, t);
}

extern "C" int rsm_stage_order(rsm_ctx *c, int16_t *disp, int W, int H, const rsm_boundary *own) {
    if (!stage_ok(c, W, H) || !disp || !own) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    StageArgs a = one_dir(c, W, H, 0, own, nullptr);
    a.d[0].d16_in = a.d[0].d16_out = t.up(disp, px);
    if (!t.ok) return finish(c, t);
    const hipError_t oe = launch_order(a, c->stream);
    if (oe != hipSuccess) {
        (void)finish(c, t);
        return set_err(c, RSM_E_HIP, "OrderConstraint: a margin row of %d columns does not fit the LDS: %s", own->XR - own->XL + 1,
                       hipGetErrorString(oe));
    }
    t.down(disp, a.d[0].d16_in, px);
    return finish(c, t);
}

template <typename T, typename Launch>
static int uniqueness_pass(rsm_ctx *c, T *p, const T *q, int W, int H, const rsm_boundary *own, const rsm_boundary *oth, Launch launch) {
    if (!stage_ok(c, W, H) || !p || !q || !own || !oth) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    T *dp = t.up(p, px);
    T *dq = t.up(q, px);
    if (!t.ok) return finish(c, t);
    launch(dp, dq, W, H, to_mg(*own), to_mg(*oth), c->stream);
    t.down(p, dp, px);
    return finish(c, t);
}
extern "C" int rsm_stage_uniqueness_pass_s16(rsm_ctx *c, int16_t *p, const int16_t *q, int W, int H,
                                             const rsm_boundary *own, const rsm_boundary *oth) {
    return uniqueness_pass(c, p, q, W, H, own, oth, launch_uniq_s16);
}
extern "C" int rsm_stage_uniqueness_pass_f64(rsm_ctx *c, double *p, const double *q, int W, int H,
                                             const rsm_boundary *own, const rsm_boundary *oth) {
    return uniqueness_pass(c, p, q, W, H, own, oth, launch_uniq_f64);
}

extern "C" int rsm_stage_set_boundary(rsm_ctx *c, const int16_t *disp, const uint8_t *mask_own, int W, int H,
                                      const rsm_boundary *own, const rsm_boundary *oth, int16_t *BL, int16_t *BR) {
    if (!stage_ok(c, W, H) || !disp || !mask_own || !own || !oth || !BL || !BR) return RSM_E_INVALID;
    if (degenerate(to_mg(*own))) return set_err(c, RSM_E_DEGENERATE_MARGIN, "YL>=YR || XL>=XR");
    Tmp t(c);
    const size_t px = (size_t)W * H;
    StageArgs a = one_dir(c, W, H, 0, own, oth);
    a.d[0].d16_in = t.up(disp, px);
    a.d[0].mask_own = t.up(mask_own, px);
    a.d[0].BL = t.alloc<int16_t>(px);
    a.d[0].BR = t.alloc<int16_t>(px);
    a.rf_list = t.alloc<uint32_t>(SETB_SCRATCH(W));
    if (!t.ok) return finish(c, t);
    launch_fill_i16(a.d[0].BL, px, (int16_t)-10000, c->stream);
    launch_fill_i16(a.d[0].BR, px, (int16_t)10000, c->stream);
    launch_set_boundary(a, c->stream);
    t.down(BL, a.d[0].BL, px);
    t.down(BR, a.d[0].BR, px);
    return finish(c, t);
}

extern "C" int rsm_stage_rematch(rsm_ctx *c, const uint8_t *img_own, const uint8_t *img_oth, const uint8_t *mask_own,
                                 const uint8_t *mask_oth, int W, int H, int r, const rsm_boundary *own,
                                 const rsm_boundary *oth, int16_t *disp) {
    if (!stage_ok(c, W, H) || !img_own || !img_oth || !mask_own || !mask_oth || !own || !oth || !disp) return RSM_E_INVALID;
    if (degenerate(to_mg(*own))) return set_err(c, RSM_E_DEGENERATE_MARGIN, "YL>=YR || XL>=XR");
    Tmp t(c);
    const size_t px = (size_t)W * H;
    MatchBufs b{};
    if (!setup_match(c, t, img_own, img_oth, mask_own, mask_oth, W, H, r, b)) return finish(c, t);
    StageArgs a = one_dir(c, W, H, r, own, oth);
    bind_match(a, b);
    a.d[0].d16_in = a.d[0].d16_out = t.up(disp, px);
    a.d[0].BL = t.alloc<int16_t>(px);
    a.d[0].BR = t.alloc<int16_t>(px);
    if (!t.ok) return finish(c, t);
    launch_set_boundary(a, c->stream, true);
    launch_ncc_argmax(a, 2, c->stream);
    t.down(disp, a.d[0].d16_in, px);
    return finish(c, t);
}

extern "C" int rsm_stage_median(rsm_ctx *c, int16_t *disp, const uint8_t *mask_own, int W, int H,
                                const rsm_boundary *own) {
    if (!stage_ok(c, W, H) || !disp || !mask_own || !own) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    StageArgs a = one_dir(c, W, H, 0, own, nullptr);
    a.d[0].d16_in = t.up(disp, px);
    a.d[0].mask_own = t.up(mask_own, px);
    a.d[0].d16_out = t.alloc<int16_t>(px);
    if (!t.ok) return finish(c, t);
    launch_fill_i16(a.d[0].d16_out, px, (int16_t)NOMATCH, c->stream);
    launch_median(a, c->stream);
    t.down(disp, a.d[0].d16_out, px);
    return finish(c, t);
}

// The specified exp(-t) of DisparityRefine's smoothness weights (k_refine.hip: exp_neg) on an array: lets the parity
// tests hold the device evaluation to the oracle's bit for bit over the whole argument range.
static int stage_exp_neg(rsm_ctx *c, const double *t_in, int64_t n, double *out, int small_form) {
    if (!c || !t_in || !out || n < 0) return RSM_E_INVALID;
    if (n == 0) return RSM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_err(c, RSM_E_HIP, "hipSetDevice");
    Tmp t(c);
    const double *dt = t.up(t_in, (size_t)n);
    double *dout = t.alloc<double>((size_t)n);
    if (!t.ok) return finish(c, t);
    launch_exp_neg(dt, dout, (long long)n, c->stream, small_form);
    t.down(out, dout, (size_t)n);
    return finish(c, t);
}
extern "C" int rsm_stage_exp_neg(rsm_ctx *c, const double *t_in, int64_t n, double *out) { return stage_exp_neg(c, t_in, n, out, 0); }
// the form the time-skewed kernel's common path uses (no special-case code) on every argument below 512, the general one elsewhere
extern "C" int rsm_stage_exp_neg_small(rsm_ctx *c, const double *t_in, int64_t n, double *out) { return stage_exp_neg(c, t_in, n, out, 1); }

// k_refine_skew's unscaled division beside the compiler's (k_refine.hip: div_unscaled) on arrays of operands
extern "C" int rsm_stage_div_unscaled(rsm_ctx *c, const double *a_in, const double *b_in, int64_t n, double *q_fast, double *q_ieee) {
    if (!c || !a_in || !b_in || !q_fast || !q_ieee || n < 0) return RSM_E_INVALID;
    if (n == 0) return RSM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_err(c, RSM_E_HIP, "hipSetDevice");
    Tmp t(c);
    const double *da = t.up(a_in, (size_t)n), *db = t.up(b_in, (size_t)n);
    double *df = t.alloc<double>((size_t)n), *di = t.alloc<double>((size_t)n);
    if (!t.ok) return finish(c, t);
    launch_div_unscaled(da, db, df, di, (long long)n, c->stream);
    t.down(q_fast, df, (size_t)n);
    t.down(q_ieee, di, (size_t)n);
    return finish(c, t);
}

// the cloud filter's trimmed sqrtf (knn_select.h: sqrtf_rn) against the compiler's on the floats with bit patterns first .. first + n - 1
extern "C" int rsm_stage_sqrt_check(rsm_ctx *c, uint32_t first_bits, int64_t n, int64_t *mismatches) {
    if (!c || !mismatches || n < 0 || (uint64_t)first_bits + (uint64_t)n > (1ull << 32)) return RSM_E_INVALID;
    *mismatches = 0;
    if (n == 0) return RSM_OK;
    if (hipSetDevice(c->device) != hipSuccess) return set_err(c, RSM_E_HIP, "hipSetDevice");
    Tmp t(c);
    unsigned long long *d = t.alloc<unsigned long long>(1);
    if (!t.ok) return finish(c, t);
    if (hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream) != hipSuccess) return set_err(c, RSM_E_HIP, "hipMemsetAsync");
    launch_sqrt_check(first_bits, (long long)n, d, c->stream);
    unsigned long long h = 0;
    t.down(&h, d, 1);
    const int rc = finish(c, t);
    *mismatches = (int64_t)h;
    return rc;
}

// the wide-window passes' candidate split (win_index.h) against the device's / and % on every candidate of an ncx x ncy window
extern "C" int rsm_stage_win_index_check(rsm_ctx *c, int ncx, int ncy, int64_t *mismatches) {
    if (!c || !mismatches || ncx < 1 || ncy < 1 || (int64_t)ncx * ncy >= (1ll << 31)) return RSM_E_INVALID;
    *mismatches = 0;
    if (hipSetDevice(c->device) != hipSuccess) return set_err(c, RSM_E_HIP, "hipSetDevice");
    Tmp t(c);
    unsigned long long *d = t.alloc<unsigned long long>(1);
    if (!t.ok) return finish(c, t);
    if (hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream) != hipSuccess) return set_err(c, RSM_E_HIP, "hipMemsetAsync");
    launch_win_index_check(ncx, ncy, d, c->stream);
    unsigned long long h = 0;
    t.down(&h, d, 1);
    const int rc = finish(c, t);
    *mismatches = (int64_t)h;
    return rc;
}

// DisparityRefine's matching costs xi (CStereoMatching.cpp:624-629) as the device restatements of the data term compute them:
// lets the parity tests hold them to the compiled reference's own values (tests/golden: xi_table_*), bit for bit.
extern "C" int rsm_stage_refine_xi(rsm_ctx *c, const uint8_t *img_own, const uint8_t *img_oth, int W, int H, int form, double *out) {
    if (!stage_ok(c, W, H) || !img_own || !img_oth || !out || W < 3 || H < 3 || form < 0 || form > 2) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H, n = (size_t)(H - 2) * (W - 2) * (W - 2);
    const uint8_t *io = t.up(img_own, px * 3), *it = t.up(img_oth, px * 3);
    uint32_t *i4o = t.alloc<uint32_t>(px), *i4t = t.alloc<uint32_t>(px);
    double *dout = t.alloc<double>(3 * n);
    if (!t.ok) return finish(c, t);
    launch_bgr_to_bgrx(io, W, H, i4o, c->stream);
    launch_bgr_to_bgrx(it, W, H, i4t, c->stream);
    launch_refine_xi(i4o, i4t, W, H, form, dout, c->stream);
    t.down(out, (const double *)dout, 3 * n);
    return finish(c, t);
}

extern "C" int rsm_stage_cloud(rsm_ctx *c, const double *disp, const uint8_t *mask_org, const uint8_t *img_own, int W,
                               int H, const double *Q, double scale, const double *R_final, const double *T_final,
                               const rsm_boundary *own, double *xyz, uint8_t *bgr, int64_t max_points,
                               int64_t *n_points) {
    if (!stage_ok(c, W, H) || !disp || !mask_org || !img_own || !Q || !R_final || !T_final || !own || !n_points)
        return RSM_E_INVALID;
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
    const int64_t cap = max_points > 0 ? max_points : 0;
    double *dx = (xyz && cap) ? t.alloc<double>((size_t)cap * 3) : nullptr;
    uint8_t *db = (bgr && cap) ? t.alloc<uint8_t>((size_t)cap * 3) : nullptr;
    if (!t.ok) return finish(c, t);
    launch_bad_prefix(dm, W, H, pre, c->stream);
    uint8_t *fl = t.alloc<uint8_t>(px + CLOUD_BLOCKS(W, H));
    if (!t.ok) return finish(c, t);
    launch_bad_blocks(pre, W, H, fl + px, c->stream);
    launch_cloud(dd, pre, di, W, H, ksize, d1, d2, dq, dR, dT, to_mg(*own), fl, fl + px, rc, ro, dn, dx, db, cap, c->stream);
    int64_t n = 0;
    t.down(&n, (const int64_t *)dn, 1);
    *n_points = n;
    const int64_t m = n < cap ? n : cap;
    if (m > 0 && dx) t.down(xyz, (const double *)dx, (size_t)m * 3);
    if (m > 0 && db) t.down(bgr, (const uint8_t *)db, (size_t)m * 3);
    return finish(c, t);
}

extern "C" int rsm_stage_rect_map(rsm_ctx *c, const double *A, const double *R, const double *newA, int W, int H,
                                  int16_t *map1, uint16_t *map2) {
    if (!stage_ok(c, W, H) || !A || !R || !newA || !map1 || !map2) return RSM_E_INVALID;
    // (newA * R)^-1 through the same host routine the pipeline uses
    double AR[9], ir[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) AR[3 * i + j] = newA[3 * i] * R[j] + newA[3 * i + 1] * R[3 + j] + newA[3 * i + 2] * R[6 + j];
    rectify_inv3(AR, ir);
    Tmp t(c);
    const size_t px = (size_t)W * H;
    int16_t *d1 = t.alloc<int16_t>(px * 2);
    uint16_t *d2 = t.alloc<uint16_t>(px);
    if (!t.ok) return finish(c, t);
    launch_rect_map(ir, A[0], A[4], A[2], A[5], W, H, d1, d2, c->stream);
    t.down(map1, (const int16_t *)d1, px * 2);
    t.down(map2, (const uint16_t *)d2, px);
    return finish(c, t);
}

extern "C" int rsm_stage_remap(rsm_ctx *c, const uint8_t *src, int Ws, int Hs, int ch, const int16_t *map1,
                               const uint16_t *map2, int W, int H, uint8_t *dst) {
    if (!stage_ok(c, W, H) || !src || !map1 || !map2 || !dst || Ws <= 0 || Hs <= 0 || (ch != 1 && ch != 3)) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    uint8_t *ds = t.up(src, (size_t)Ws * Hs * ch);
    int16_t *d1 = t.up(map1, px * 2);
    uint16_t *d2 = t.up(map2, px);
    uint8_t *dd = t.alloc<uint8_t>(px * ch);
    if (!t.ok) return finish(c, t);
    launch_remap(ds, Ws, Hs, ch, d1, d2, W, H, dd, c->stream);
    t.down(dst, (const uint8_t *)dd, px * ch);
    return finish(c, t);
}

extern "C" int rsm_stage_erode_gray(rsm_ctx *c, const uint8_t *src, int W, int H, int ksize, uint8_t *dst) {
    if (!stage_ok(c, W, H) || !src || !dst || ksize < 1 || ksize > 255) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    std::vector<int> j1, j2;
    ellipse_spans(ksize, j1, j2);
    uint8_t *ds = t.up(src, px);
    int *d1 = t.up(j1.data(), (size_t)ksize), *d2 = t.up(j2.data(), (size_t)ksize);
    uint8_t *stb = t.alloc<uint8_t>(px * 9), *dd = t.alloc<uint8_t>(px);
    if (!t.ok) return finish(c, t);
    launch_erode_gray(ds, W, H, ksize, d1, d2, stb, dd, c->stream);
    t.down(dst, (const uint8_t *)dd, px);
    return finish(c, t);
}

// ---- NCC kernel microbenchmark --------------------------------------------------------------------
extern "C" int rsm_bench_ncc(rsm_ctx *c, int W, int H, int r, int cands, int iters, double *ms_per_launch) {
    if (!stage_ok(c, W, H) || r < 1 || r > 15 || cands < 1 || iters < 1 || !ms_per_launch) return RSM_E_INVALID;
    if (W <= 2 * r + cands + 2 || H <= 2 * r + 2) return RSM_E_INVALID;
    Tmp t(c);
    const size_t px = (size_t)W * H;
    std::vector<uint8_t> hi(px * 3), hm(px, 255);
    uint32_t s = 12345u;
    for (auto &v : hi) {
        s = s * 1664525u + 1013904223u;
        v = (uint8_t)(s >> 24);
    }
    MatchBufs b{};
    if (!setup_match(c, t, hi.data(), hi.data(), hm.data(), hm.data(), W, H, r, b)) return finish(c, t);
    rsm_boundary m{r, H - 1 - r, r, W - 1 - r, W - 2 * r, H - 2 * r};
    StageArgs a = one_dir(c, W, H, r, &m, &m);
    bind_match(a, b);
    std::vector<int16_t> hl(px), hr(px);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int L = x - cands / 2, R = L + cands - 1;
            if (L < r) { L = r; R = L + cands - 1; }
            if (R > W - 1 - r) { R = W - 1 - r; L = R - cands + 1; }
            hl[(size_t)y * W + x] = (int16_t)L;
            hr[(size_t)y * W + x] = (int16_t)R;
        }
    a.d[0].BL = t.up(hl.data(), px);
    a.d[0].BR = t.up(hr.data(), px);
    int16_t *dd = t.alloc<int16_t>(px);
    const int uploaded = finish(c, t); // hi, hm, hl, hr are read: an early return below may let them go
    if (uploaded != RSM_OK) return uploaded;
    a.d[0].d16_in = a.d[0].d16_out = dd;
    launch_fill_i16(dd, px, (int16_t)NOMATCH, c->stream);
    launch_ncc_argmax(a, 1, c->stream); // warm-up (setup_match zeroed the counter)
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0));
    HIPCHK(c, hipEventCreate(&e1));
    HIPCHK(c, hipEventRecord(e0, c->stream));
    for (int i = 0; i < iters; i++) {
        (void)hipMemsetAsync(a.ncc_cnt, 0, sizeof(int), c->stream); // fresh wide-pixel counter per launch
        (void)hipMemsetAsync(a.tie_cnt, 0, 2 * sizeof(int), c->stream);
        (void)hipMemsetAsync(a.wrow, 0, sizeof(int32_t) * (size_t)H, c->stream);
        launch_ncc_argmax(a, 1, c->stream);
    }
    HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_launch = (double)ms / iters;
    return finish(c, t);
}
