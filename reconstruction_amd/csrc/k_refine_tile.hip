// k_refine_tile.hip -- DisparityRefine's Jacobi sweeps (CStereoMatching.cpp:590-678) on the SMALL levels, T per launch on
// overlapped tiles (the values are those of T single sweeps, bit for bit).
//
// A small level's single sweep is a few microseconds of work behind a launch that takes longer than that, and a level runs 30
// to 120 of them, each waiting for the one before: the levels below the time-skewed kernel's (k_refine_skew.hip) are bound by
// launch latency.  This kernel buys launches with redundant arithmetic.  A workgroup owns a TL_TX x TL_TY tile of a direction's
// interior, stages the tile grown by T pixels on every side (clipped to the margin box: border and NOMATCH pixels are never
// updated, .cpp:592,608,613, so nothing outside the box is needed) and runs T sweeps on it without talking to any other
// workgroup: sweep s computes the tile grown by T - s, everything else copies through, one workgroup barrier per sweep.  The
// state ping-pongs between two LDS planes; a thread keeps its pixels' key dwords and both ways' cache entries in registers.
// All global loads go out in one batch up front; the owned pixels go to f64_b at the end.
//
// The update is refine_update and the miss service rf_serve_misses (per wave through an LDS list), the single sweep kernel's
// too: no new formulation of the arithmetic.  A new entry lives in the
// thread's registers for the rest of the launch; those of OWNED pixels go to the update list that k_refine_apply scatters
// after the launch, at most one record per (pixel, way) and launch, exactly as k_refine_skew does it (a neighbouring tile may
// be staging that pixel at the same moment: an in-place write could be read torn).  A full list drops the record, which costs
// a later miss and never bits; halo pixels' new entries are never written back.
#include "refine_common.h"

typedef unsigned long long u64;

#define TL_TX 32
#define TL_TY 16

template <int T>
__global__ __launch_bounds__(256) void k_refine_tile(StageArgs a) {
    constexpr int RW = TL_TX + 2 * T, RH = TL_TY + 2 * T; // the staged region
    constexpr int NPIX = RW * RH, PPT = (NPIX + 255) / 256; // thread `tid` holds the region pixels i * 256 + tid
    constexpr int CAP = 64 * PPT;                            // every pixel of a wave may miss
    __shared__ double s_d[2][NPIX];
    __shared__ uint32_t s_list[4][CAP]; // region pixel | (iMatch - x) << 16
    __shared__ double2 s_res[4][CAP];
    __shared__ double2 s_exp[128]; // the specified exp's table (exp_tab_stage)
    exp_tab_stage(s_exp);
    const DirArgs &d = a.d[blockIdx.z];
    const int W = a.W, H = a.H;
    const int XL = d.own.XL, XR = d.own.XR, YL = d.own.YL, YR = d.own.YR;
    const int gx0 = XL + 1 + (int)blockIdx.x * TL_TX - T, gy0 = YL + 1 + (int)blockIdx.y * TL_TY - T; // the region's corner
    if (gx0 + T > XR - 1 || gy0 + T > YR - 1) return; // workgroup-uniform: no interior pixel to own
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const double NM = (double)NOMATCH;

    // ---- staging: one batch of loads
    int pix[PPT], lim[PPT]; // the pixel's index in the level; the last sweep of the launch that computes it (0: none -- outside
                            // the interior; T: an owned pixel)
    uint32_t kk[PPT];
    double2 e0[PPT], e1[PPT];
    double st0[PPT];
#pragma unroll
    for (int i = 0; i < PPT; i++) {
        const int p = i * 256 + tid;
        const int rx = p % RW, ry = p / RW, x = gx0 + rx, y = gy0 + ry;
        const bool inbox = p < NPIX && x >= XL && x <= XR && y >= YL && y <= YR;
        const bool inner = inbox && x > XL && x < XR && y > YL && y < YR;
        lim[i] = inner ? min(min(min(rx, RW - 1 - rx), min(ry, RH - 1 - ry)), T) : 0; // (the region's edge is T away from the tile)
        pix[i] = inbox ? y * W + x : 0;
        st0[i] = NM;
        kk[i] = RF_NOKEY2;
        e0[i] = e1[i] = make_double2(0.0, 0.0);
        if (inbox) st0[i] = d.f64_a[pix[i]];
        if (lim[i] > 0) {
            kk[i] = d.rf_key[pix[i]];
            e0[i] = d.rf_ent[pix[i]];
            e1[i] = d.rf_ent[(size_t)pix[i] + a.rf_stride];
        }
    }
    bool any = false;
#pragma unroll
    for (int i = 0; i < PPT; i++) {
        const int p = i * 256 + tid;
        if (p < NPIX) s_d[0][p] = st0[i];
        any |= lim[i] == T && st0[i] != NM;
    }
    if (!__syncthreads_or(any)) return; // workgroup-uniform: no live pixel in the tile (outside an elliptic mask, a hole)

    RfUpd *upd;
    int32_t *cnt;
    rf_upd_shard(a, rf_upd_wg_shard(), upd, cnt);
    const u64 below = (1ull << lane) - 1ull;
    unsigned listed = 0; // bit 2 i + way: this launch has listed a new entry for that cache slot

#pragma unroll 1
    for (int s = 1; s <= T; s++) {
        const double *cur = s_d[(s - 1) & 1];
        double *nxt = s_d[s & 1];
        // a pixel this sweep does not compute reads the neighbours of region pixel (1, 1) instead of its own (which may lie
        // outside the planes) and ignores them
        auto fetch = [&](int i, double &dC, double &dE, double &dW, double &dN, double &dS, int &mode) -> bool {
            const int p = i * 256 + tid;
            const bool act = s <= lim[i];
            dC = cur[p < NPIX ? p : 0];
            const int pa = act ? p : RW + 1;
            dE = cur[pa + 1], dW = cur[pa - 1], dN = cur[pa - RW], dS = cur[pa + RW];
            mode = refine_mode(dE, dW, dN, dS);
            return act && dC != NM && mode != 0; // .cpp:613 (mode 0 copies through, .cpp:655)
        };
        // (1) the misses of this wave's pixels, compacted
        unsigned need = 0, miss = 0;
        int rel[PPT], pos[PPT];
        int n = 0; // uniform
#pragma unroll
        for (int i = 0; i < PPT; i++) {
            double dC, dE, dW, dN, dS;
            int mode;
            const bool nd = fetch(i, dC, dE, dW, dN, dS, mode);
            rel[i] = (int)(dC - 1.5); // .cpp:625 (iMatch - x)
            const bool ms = nd && rf_key_get(kk[i], rel[i]) != rel[i];
            const u64 mm = __ballot(ms);
            pos[i] = n + __popcll(mm & below);
            if (ms) s_list[wid][pos[i]] = rf_miss_entry(i * 256 + tid, rel[i]);
            n += __popcll(mm);
            need |= (unsigned)nd << i;
            miss |= (unsigned)ms << i;
        }
        if (n) { // wave-uniform
            // (2) served per wave
            rf_serve_misses(
                s_list[wid], n, lane, &d, W, H,
                [&](uint32_t en, int &ex, int &ey, int &r) { ex = gx0 + rf_miss_slot(en) % RW, ey = gy0 + rf_miss_slot(en) / RW, r = rf_miss_rel(en); },
                [&](int e, int, int, int, double pw, double dl) { s_res[wid][e] = make_double2(pw, dl); });
            // (3) the new entries into the registers; those of owned pixels to the update list, once per (pixel, way)
            u64 bm[PPT];
            unsigned emit = 0;
            int tot = 0;
#pragma unroll
            for (int i = 0; i < PPT; i++) {
                const int way = rel[i] & 1;
                const bool ms = (miss >> i) & 1u;
                if (ms) {
                    const double2 pd = s_res[wid][pos[i]];
                    if (way) e1[i] = pd;
                    else e0[i] = pd;
                    kk[i] = rf_key_put(kk[i], rel[i]);
                }
                const bool em = ms && lim[i] == T && !((listed >> (2 * i + way)) & 1u);
                bm[i] = __ballot(em);
                tot += __popcll(bm[i]);
                emit |= (unsigned)em << i;
            }
            if (tot) { // wave-uniform
                int base = 0;
                if (lane == 0) base = atomicAdd(cnt, tot);
                base = __shfl(base, 0);
#pragma unroll
                for (int i = 0; i < PPT; i++) {
                    const int way = rel[i] & 1;
                    const int at = base + __popcll(bm[i] & below);
                    if (((emit >> i) & 1u) && at < a.upd_cap) {
                        upd[at] = rf_upd_record((uint32_t)pix[i], blockIdx.z, rel[i], way ? e1[i] : e0[i]);
                        listed |= 1u << (2 * i + way);
                    }
                    base += __popcll(bm[i]);
                }
            }
        }
        // (4) the sweep
#pragma unroll
        for (int i = 0; i < PPT; i++) {
            const int p = i * 256 + tid;
            double dC, dE, dW, dN, dS;
            int mode;
            fetch(i, dC, dE, dW, dN, dS, mode);
            double val = dC;
            if ((need >> i) & 1u) {
                const double2 pd = (rel[i] & 1) ? e1[i] : e0[i];
                val = refine_update(mode, dC, dE, dW, dN, dS, pd.x, pd.y, a.ws, s_exp);
            }
            if (p < NPIX) nxt[p] = val;
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < PPT; i++) {
        const int p = i * 256 + tid;
        if (lim[i] != T) continue; // not owned
        const double v = s_d[T & 1][p];
        if (v != NM) d.f64_b[pix[i]] = v;
    }
}

// T sweeps f64_a -> f64_b in one launch on overlapped tiles (a.rf_launch = launch index: the update list's counter set) + the
// launch that applies its cache updates.  T in 2 .. RF_TILE_MAXT.
void launch_refine_tile(const StageArgs &a, int T, hipStream_t st) {
    int rows, cols;
    if (!refine_interior(a, rows, cols) || T < 2 || T > RF_TILE_MAXT) return;
    const dim3 grid((cols + TL_TX - 1) / TL_TX, (rows + TL_TY - 1) / TL_TY, a.ndir);
    switch (T) {
#define RF_LAUNCH(TT) \
    case TT: hipLaunchKernelGGL(k_refine_tile<TT>, grid, dim3(256), 0, st, a); break
        RF_LAUNCH(2);
        RF_LAUNCH(3);
        RF_LAUNCH(4);
        RF_LAUNCH(5);
        RF_LAUNCH(6);
        RF_LAUNCH(7);
        RF_LAUNCH(8);
#undef RF_LAUNCH
    }
    launch_refine_apply(a, st);
}
