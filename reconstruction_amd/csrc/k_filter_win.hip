// k_filter_win.hip -- the cloud filter's k-nearest search on the pixel lattice (the host steps that run it: k_filter.hip).
// Pixel-window k nearest (rsm_filter_last_cloud, round 5): the cloud of a matched pair is a DEPTH MAP -- point i sits on
// the ray of its pixel, P = iW (x + q03, y + q13, qz) before the rigid R_final / T_final (DisparityToCloud,
// CStereoMatching.cpp:732-749) -- so the pixel lattice itself is the search structure: the k nearest of a point are among
// the points of the (2 WR + 1)^2 pixels around its own, PROVIDED the (k+1)-th smallest distance found there is below the
// distance from P to every ray OUTSIDE that window.  For a ray through pixel offset (a, b), rho = |(a, b)| >= WR + 1:
//     dist(P, ray) = |iW| |D x D'| / |D'| >= |iW| |qz| rho / (|D| + rho),   D = (x + q03, y + q13, qz), D' = D + (a, b, 0)
// (|D x D'|^2 = qz^2 rho^2 + (Dx b - Dy a)^2, |D'| <= |D| + rho), increasing in rho, so with |iW| |qz| = |F2| (the point's
// depth in the camera frame) and |iW| |D| = |P - T|:
//     LB = |F2| (WR + 1) / (|P - T| |qz| / |F2| + WR + 1).
// A query whose (k+1)-th smallest float32 distance stays below LB minus a rounding margin is decided HERE with exactly the
// values the generic search would find (same float32 squared distances, the k smallest by value, the same exact double
// sum); every other query -- near a depth edge, a hole, the mask's border, an outlier: the thick or thin parts of the
// sheet -- is flagged and goes to the grid ladder (k_filter.hip).  The selection is per LANE (a query per thread, a 32 x 8 tile of
// pixels per workgroup, the tile and its halo in LDS as float4): pass 1 bins the window's squared distances into 32
// per-thread LDS counters over [0, 4 tau_est] (tau_est = the (k+1)/pi lateral spacings^2 of a fronto-parallel sheet), the
// scan finds the bin holding rank k + 1, pass 2 sums sqrt(d2) of the bins below it in double (in window order: a query is decided
// here only if knn_sum_exact says that no addition rounded, so that the order is no choice) and lists
// the few values of that bin, whose rank-th smallest is tau.  ~120 wave-instructions per query against ~2000 of the
// wave-per-query grid search.
// (The bound and its margins: win_bound.h.)
#include "filter_units.h"
#include "knn_select.h"
#include "win_index.h"

#include <algorithm>

#define WIN_TX 32
#define WIN_TY 8
#define WIN_NB 32   // distance bins per query over [0, bound^2): the rank's bin holds ~1.5 (k + 1) / (its index) values, a handful
#define WIN_LCAP 24 // values of the rank's bin a query can list (more: undecided -> the ladder); the list reuses the counters' LDS
// (WIN_DRAIN_W and WIN_TILE_CH are build knobs: make EXTRA_k_filter_win="-DWIN_TILE_CH=11", tests/tools/build_variants_tu.sh k_filter_win ...)
#ifndef WIN_DRAIN_W
#define WIN_DRAIN_W 4 // waiting values whose square roots are taken together (reads in flight together, sequences interleaved)
#endif
#ifndef WIN_TILE_CH
#define WIN_TILE_CH 9 // candidates per chunk of the tile form (two register buffers of that many 16-byte entries)
#endif

// lattice copy of the cloud: float4 (x, y, z as InsertPoint keeps them, bits of the point index) per flagged pixel of the
// margin's box, NaN elsewhere (the buffer is pre-filled); block = row, the compaction order of k_cloud<1>
__global__ __launch_bounds__(256) void k_cloud_lattice(const uint8_t *__restrict__ flags, const int64_t *__restrict__ row_offset, int W, int XL, int XR, int YL,
                                                        const double *__restrict__ xyz, int64_t n, int gw, float4 *__restrict__ lat,
                                                        unsigned int *__restrict__ cell_of) {
    __shared__ int s_w[4];
    __shared__ long long s_base;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int y = YL + blockIdx.x;
    if (tid == 0) s_base = (long long)row_offset[blockIdx.x];
    __syncthreads();
    for (int x0 = XL; x0 <= XR; x0 += 256) {
        const int x = x0 + tid;
        const bool f = (x <= XR) && flags[(size_t)y * W + x];
        const unsigned long long b = __ballot(f);
        if (lane == 0) s_w[wid] = __popcll(b);
        __syncthreads();
        if (f) {
            long long pos = s_base + __popcll(b & ((1ull << lane) - 1ull));
            for (int w = 0; w < wid; w++) pos += s_w[w];
            if (pos < n) {
                const float px = (float)xyz[3 * pos], py = (float)xyz[3 * pos + 1], pz = (float)xyz[3 * pos + 2]; // InsertPoint's cast
                const size_t cell = (size_t)(blockIdx.x + WIN_PAD) * gw + (x - XL + WIN_PAD);
                cell_of[pos] = (unsigned int)cell;
                if (isfinite(px) && isfinite(py) && isfinite(pz)) // (non-finite points take no part in the searches)
                    lat[cell] = make_float4(px, py, pz, __uint_as_float((unsigned int)pos));
            }
        }
        __syncthreads();
        if (tid == 0) s_base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

// One query of the pixel-window search: P = the query's lattice entry, ld(r, c) = the lattice entry at window row r / column c
// (0 .. 2 WR), col = the thread's private LDS column (stride 256 words: WIN_NB + 1 words of counters, later the list), CH = the
// candidates whose reads are in flight together (a divisor of 2 WR + 1).  Returns whether the query is decided; *out = its mean
// neighbour distance, *lim_out = the bound.
// The pixels a window of "radius" WR has to look at: the bound holds for every ray at a pixel distance rho >= WR + 1, so the DISC
// a^2 + b^2 <= (WR + 1)^2 - 1 suffices -- the corners of the square are farther than the rays the bound already covers.  The rows
// of the window fall into four classes by |b| (<= WR/2, <= 3WR/4, <= 7WR/8, <= WR), each as wide as its widest row needs: 14 %
// fewer candidates than the square at WR = 16 (937 of 1089), the code of a row four times.
constexpr int win_isqrt(int v) {
    int r = 0;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}
constexpr int win_halfwidth(int WR, int b) { // widest |a| of the disc's row b, at most WR
    const int a = win_isqrt((WR + 1) * (WR + 1) - 1 - b * b);
    return a < WR ? a : WR;
}
// a row of wd candidates in nch chunks: the first wd % nch one longer
template <int wd, int nch>
struct WinSplit {
    static constexpr int nmax = (wd + nch - 1) / nch;
    static constexpr int size(int j) { return wd / nch + (j < wd % nch ? 1 : 0); }
    static constexpr int off(int j) {
        int o = 0;
        for (int i = 0; i < j; i++) o += size(i);
        return o;
    }
};
template <int WR, int CH, class Loader>
__device__ __forceinline__ bool win_query(const Loader &ld, const float4 P, const WinGeom &g, int mean_k, unsigned int *col, float *out, double *lim_out) {
    constexpr int NC = 2 * WR + 1;
    (void)NC;
    const WinBound bound = win_bound(P, g, WR);
    *lim_out = bound.lim;
    const float range = bound.range; // tau must stay below this; the bins cover [0, range)
    const int want = mean_k + 1;
    const float inv_w = (range > 0.0f) ? (float)WIN_NB / range : 0.0f;
    if (!(range > 0.0f && inv_w > 0.0f && isfinite(inv_w))) return false;
    // bin of a squared distance: 0 .. WIN_NB - 1 below the bound, WIN_NB (the sink row) at or beyond it and for NaN (a pixel without a
    // point: fminf returns the other operand) -- monotone in d2; one multiply, one minimum, one conversion
    auto bin_of = [&](float d2) { return (int)fminf(d2 * inv_w, (float)WIN_NB); };
    // A chunk of a window row at a time: all its reads first (16-byte reads, in flight together), then the arithmetic -- a read,
    // its wait and a data-dependent branch per candidate would expose the read latency (2 x 1089 times per query at WR = 16).
    // the squared distance of fdist2 -- (dx dx + dy dy) + dz dz, the same operations on the same operands -- with x and y as one
    // packed pair (v_pk_add_f32 / v_pk_mul_f32: the lattice entry's x and y arrive in adjacent registers)
    typedef float v2f __attribute__((ext_vector_type(2)));
    const v2f Pxy = {P.x, P.y};
    auto d2_of = [&](const float4 &o) {
        const v2f oxy = {o.x, o.y};
        const v2f dxy = Pxy - oxy;
        const v2f sq = dxy * dxy;
        const float dz = P.z - o.z;
        return (sq.x + sq.y) + dz * dz;
    };
    // The disc, a row class at a time.  A row is cut into an even number of chunks of at most CH candidates and the chunks stream
    // through two register buffers: the 16-byte reads of the NEXT chunk (of this row, or the first of the next row) are issued
    // before the arithmetic of the current one, so a wave computes while its own reads are under way (round 5 read a whole row,
    // waited, computed: with the two waves per SIMD that 75 KB of LDS leave, the vector unit idled a third of the time).
    // pre(n) before a chunk of n candidates, body(d2) per candidate; NaN for a pixel without a point: every test fails.
    auto for_disc = [&](auto &&pre, auto &&body) {
        auto rows = [&](int lo, int hi, auto hw_) { // the rows with |b| in [lo, hi] (lo = 0: one run of rows, else one above and one below), half width hw
            constexpr int hw = decltype(hw_)::value, wd = 2 * hw + 1, nch0 = (wd + CH - 1) / CH, nch = nch0 + (nch0 & 1);
            typedef WinSplit<wd, nch> S;
            float4 buf[2][S::nmax];
            auto issue = [&](auto j_, auto b_, int r) { // the reads of chunk j of window row r, into buffer b
                constexpr int j = decltype(j_)::value, bb = decltype(b_)::value;
#pragma unroll
                for (int i = 0; i < S::size(j); i++) buf[bb][i] = ld(r, WR - hw + S::off(j) + i);
            };
            auto use = [&](auto j_, auto b_) {
                constexpr int j = decltype(j_)::value, bb = decltype(b_)::value;
#pragma unroll
                for (int i = 0; i < S::size(j); i++) asm volatile("" : "+v"(buf[bb][i].w)); // (keeps the reads 16-byte ones: twice the LDS rate of the 12-byte form)
                pre(S::size(j));
#pragma unroll
                for (int i = 0; i < S::size(j); i++) body(d2_of(buf[bb][i]));
            };
            auto steps = [&](auto &&self, auto j_, int r, int rn) -> void {
                constexpr int j = decltype(j_)::value;
                if constexpr (j + 1 < nch) issue(std::integral_constant<int, j + 1>(), std::integral_constant<int, (j + 1) & 1>(), r);
                else issue(std::integral_constant<int, 0>(), std::integral_constant<int, 0>(), rn);
                __builtin_amdgcn_sched_barrier(0); // (the reads stay ahead of the arithmetic)
                use(j_, std::integral_constant<int, j & 1>());
                if constexpr (j + 1 < nch) self(self, std::integral_constant<int, j + 1>(), r, rn);
            };
#pragma unroll 1
            for (int run = 0; run < (lo == 0 ? 1 : 2); run++) {
                const int r0 = lo == 0 ? WR - hi : (run ? WR + lo : WR - hi), r1 = lo == 0 ? WR + hi : (run ? WR + hi : WR - lo);
                issue(std::integral_constant<int, 0>(), std::integral_constant<int, 0>(), r0);
#pragma unroll 1
                for (int r = r0; r <= r1; r++) steps(steps, std::integral_constant<int, 0>(), r, r + (r < r1 ? 1 : 0)); // (after the last row: its first chunk once more, unused)
            }
        };
        constexpr int g1 = WR / 2, g2 = 3 * WR / 4, g3 = 7 * WR / 8;
        rows(0, g1, std::integral_constant<int, win_halfwidth(WR, 0)>());
        if (g2 > g1) rows(g1 + 1, g2, std::integral_constant<int, win_halfwidth(WR, g1 + 1)>());
        if (g3 > g2) rows(g2 + 1, g3, std::integral_constant<int, win_halfwidth(WR, g2 + 1)>());
        if (WR > g3) rows(g3 + 1, WR, std::integral_constant<int, win_halfwidth(WR, g3 + 1)>());
    };
    // pass 1: histogram of the window's squared distances (the point itself included: d2 = 0, as nearestKSearch(k + 1)); branch-free:
    // what lies beyond the bound goes to the sink row
    for_disc([](int) {}, [&](float d2) {
        const int b = bin_of(d2);
        atomicAdd(col + 256 * b, 1u); // (no return value: a fire-and-forget ds_add)
    });
    // the bin holding rank `want` (all counters read first: one LDS round trip, not one per bin)
    int below = 0, bstar = -1, in_bin = 0;
    {
        int h[WIN_NB];
#pragma unroll
        for (int b = 0; b < WIN_NB; b++) h[b] = (int)col[256 * b];
#pragma unroll
        for (int b = 0; b < WIN_NB; b++) {
            const bool hit = bstar < 0 && below + h[b] >= want;
            bstar = hit ? b : bstar;
            in_bin = hit ? h[b] : in_bin;
            below = bstar < 0 ? below + h[b] : below;
        }
    }
    if (!(bstar >= 0 && in_bin <= WIN_LCAP)) return false; // fewer than k + 1 points within the bound in the window, or too many (nearly) equal distances
    // pass 2: the exact sum below the bin, the bin's values listed (over the counters: they are dead now).  The bin tests become
    // two float compares: t_lo / t_hi = the smallest floats whose bin is >= bstar / > bstar (bin_of is monotone).
    // A tenth of a wave's lanes has a value below t_lo per candidate, so a square root taken where the value is met runs its whole
    // sequence for a few lanes nearly every time (36 instructions per candidate, round 5).  Instead every value below t_hi WAITS in
    // the lane's own column -- rows in_bin .. WIN_NB, the rows the bin's list leaves free -- and before a chunk that some lane has
    // no room for, the wave takes the square roots of everything waiting, eight rows at a time (the reads in flight together, the
    // sequences interleaved): most lanes busy, a tenth as often.  That changes the order of the additions; the sum's bits are
    // PCL's whenever none of them rounds, which knn_sum_exact tests at the end (odd_min: the smallest positive value added).
    float *lst = (float *)col;
    double sum = 0.0;
    int nl = 0;
    unsigned int odd_min = 0xffffffffu; // tracks whether an input outside the trimmed square root's range (0 < d2 < 2^-96) was met
    auto first_in = [&](int b) { // smallest float t >= 0 with bin_of(t) >= b, b in 1 .. WIN_NB
        float t = (float)b / inv_w;
        while (t > 0.0f && bin_of(__uint_as_float(__float_as_uint(t) - 1u)) >= b) t = __uint_as_float(__float_as_uint(t) - 1u);
        while (bin_of(t) < b) t = __uint_as_float(__float_as_uint(t) + 1u);
        return t;
    };
    const float t_lo = bstar > 0 ? first_in(bstar) : 0.0f;
    const float t_hi = fminf(first_in(bstar + 1), range); // (a value at the bound's edge can round into the last bin: it is not listed, the count then disagrees and the query is left undecided)
    static_assert(WIN_NB + 1 - WIN_LCAP >= CH, "a lane's waiting rows hold at least one chunk");
    typedef __attribute__((address_space(3))) float lds_float; // (32-bit LDS addresses: a generic pointer costs 64-bit arithmetic per candidate)
    lds_float *const wait0 = (lds_float *)lst + 256 * in_bin, *const wait_end = (lds_float *)lst + 256 * (WIN_NB + 1), *const wait_last = wait_end - 256;
    lds_float *wait = wait0;
    asm volatile("" : "+v"(wait)); // (one register, not base + offset: an addition less per waiting value)
    auto drain = [&]() {
        // (the trimmed square root itself; an input it is not made for -- positive and below 2^-96: float32 coordinates do not
        // produce such differences -- marks the query `odd`, and it is left to the later passes, which take sqrtf)
#pragma unroll 1
        for (const lds_float *p = wait0; p < wait; p += WIN_DRAIN_W * 256) {
            float v[WIN_DRAIN_W];
#pragma unroll
            for (int t = 0; t < WIN_DRAIN_W; t++) v[t] = *(p + 256 * t < wait_last ? p + 256 * t : wait_last); // (rows at or beyond `wait`: read, not used)
#pragma unroll
            for (int t = 0; t < WIN_DRAIN_W; t++) {
                const bool live = p + 256 * t < wait, low = v[t] < t_lo;
                if (live && !low) { // one of the bin's own values: to the list
                    lst[min(nl, in_bin) * 256] = v[t]; // (nl <= in_bin by the histogram; the clamp keeps a disagreement inside the column -- it then
                    nl++;                              // spoils a waiting value of a query that is left undecided anyway)
                }
                const float u = live && low ? v[t] : 0.0f;       // (the square root of 0 adds nothing)
                odd_min = min(odd_min, __float_as_uint(u) - 1u); // (the smallest positive pattern met, minus one; 0 wraps to the top)
                sum += (double)sqrtf_rn_core(u);
            }
        }
        wait = wait0;
        asm volatile("" : "+v"(wait));
    };
    for_disc(
        [&](int n) {
            if (__builtin_expect(__any(wait + 256 * n > wait_end), 0)) drain();
        },
        [&](float d2) {
            if (d2 < t_hi) // below the bin or in it: waits (NaN -- a pixel without a point -- fails the test).  *wait++ = d2 with a row's stride, as
                           // the two instructions it is (the compiler adds into a temporary and copies it back: a third of this region)
            {
                *wait = d2;
                wait += 256;
            }
        });
    drain();
    // tau = the (want - below)-th smallest of the listed values (by value: ties are equal distances): the list into registers
    // (unused slots +inf), sorted by Batcher's merge exchange on the bit patterns (non-negative floats order as unsigned integers)
    const int rank = want - below; // 1 .. in_bin
    unsigned int u[WIN_LCAP];
#pragma unroll
    for (int j = 0; j < WIN_LCAP; j++) u[j] = __float_as_uint(lst[j * 256]);
#pragma unroll
    for (int j = 0; j < WIN_LCAP; j++) u[j] = j < nl ? u[j] : 0x7f800000u;
#pragma unroll
    for (int pp = 1; pp < WIN_LCAP; pp *= 2) {
#pragma unroll
        for (int k = pp; k >= 1; k /= 2) {
#pragma unroll
            for (int j = k % pp; j + k < WIN_LCAP; j += 2 * k) {
#pragma unroll
                for (int i = 0; i < (k < WIN_LCAP - j - k ? k : WIN_LCAP - j - k); i++) {
                    if ((i + j) / (2 * pp) == (i + j + k) / (2 * pp)) {
                        const unsigned int lo = min(u[i + j], u[i + j + k]), hi = max(u[i + j], u[i + j + k]);
                        u[i + j] = lo;
                        u[i + j + k] = hi;
                    }
                }
            }
        }
    }
    unsigned int tau_b = 0u;
#pragma unroll
    for (int j = 0; j < WIN_LCAP; j++) tau_b = (j == rank - 1) ? u[j] : tau_b;
    const float tau = __uint_as_float(tau_b);
    int less = 0;
#pragma unroll
    for (int j = 0; j < WIN_LCAP; j++) less += u[j] < tau_b;
#pragma unroll
    for (int j = 0; j < WIN_LCAP; j++) { // the values below tau are the first `less` of the sorted list
        if (!__any(j < less)) break;
        const float x = j < less ? __uint_as_float(u[j]) : 0.0f;
        odd_min = min(odd_min, __float_as_uint(x) - 1u);
        sum += (double)sqrtf_rn_core(x);
    }
    if (!(nl == in_bin && tau < range) || odd_min < 0x0f7fffffu) return false;
    // every point outside the window is farther than sqrt(tau): the k + 1 smallest are all here
    sum += (double)(want - (below + less)) * (double)sqrtf(tau);
    // odd_min is knn_sum_exact's min_m1 over everything added above.  A sum whose order matters (no lattice cloud produces one: DESIGN.md
    // 9 f3) is left to the later passes, which add it in PCL's order
    if (!knn_sum_exact(sum, knn_min_m1(odd_min, tau))) return false;
    *out = (float)(sum / mean_k);
    return true;
}

// Tile form: a workgroup = a 32 x 8 tile of pixels, its window halo staged in LDS, a thread = the query of its pixel.
// PROBE: every `tile_step`-th tile in x and y only, nothing written but three counters (queries seen, queries decided, the sum of
// their bounds): the host picks the smallest window radius that decides most of a sparse sample before it pays for the full pass.
template <int WR, bool PROBE>
__global__ __launch_bounds__(256) void k_sor_window(const float4 *__restrict__ lat, WinGeom g, int mean_k, float *__restrict__ dist,
                                                     unsigned int *__restrict__ undecided, int tile_step, unsigned int *__restrict__ probe_cnt) {
    constexpr int SW = WIN_TX + 2 * WR, SH = WIN_TY + 2 * WR;
    __shared__ float4 s_t[SH][SW];
    __shared__ unsigned int s_u[WIN_NB + 1][256]; // column tid is private to thread tid: first the bin counters (row WIN_NB: the sink of
                                                  // candidates beyond the bound / pixels without a point), then the list of the rank's bin
    static_assert(WIN_LCAP <= WIN_NB, "the list reuses the counters' storage");
    const int tid = threadIdx.x, tx = tid & (WIN_TX - 1), ty = tid / WIN_TX;
    const int gx0 = WIN_PAD + (int)blockIdx.x * tile_step * WIN_TX - WR, gy0 = WIN_PAD + (int)blockIdx.y * tile_step * WIN_TY - WR; // lattice position of s_t[0][0]
    for (int e = tid; e < SW * SH; e += 256) {
        const int r = e / SW, c = e - r * SW;
        const int gy = min(gy0 + r, g.gh - 1), gx = min(gx0 + c, g.gw - 1); // (the last tiles' overhang re-reads the border: NaN)
        s_t[r][c] = lat[(size_t)gy * g.gw + gx];
    }
#pragma unroll
    for (int b = 0; b <= WIN_NB; b++) s_u[b][tid] = 0u;
    __syncthreads();
    const float4 P = s_t[ty + WR][tx + WR];
    const bool valid = P.x == P.x; // NaN: no point at this pixel
    if (!__syncthreads_or(valid)) return;
    auto ld = [&](int r, int c) { return s_t[ty + r][tx + c]; };
    float res = 0.0f;
    double lim = 0.0;
    const bool ok = valid && win_query<WR, WIN_TILE_CH>(ld, P, g, mean_k, &s_u[0][tid], &res, &lim);
    if (PROBE) {
        const unsigned long long mv = __ballot(valid), mo = __ballot(ok);
        float sl = valid ? (float)fmax(lim, 0.0) : 0.0f; // the mean bound: what the queries this radius leaves over have in common (tau >= lim^2)
        for (int o = 32; o > 0; o >>= 1) sl += __shfl_xor(sl, o);
        if ((tid & 63) == 0 && mv) {
            atomicAdd(&probe_cnt[0], (unsigned int)__popcll(mv));
            atomicAdd(&probe_cnt[1], (unsigned int)__popcll(mo));
            atomicAdd((float *)&probe_cnt[2], sl);
        }
    } else if (valid) {
        if (ok) dist[__float_as_uint(P.w)] = res;
        undecided[__float_as_uint(P.w)] = ok ? 0u : 1u;
    }
}

// List form: a thread = one listed query (what the tile pass left over -- a seventh of a thick sheet's points, scattered), its
// window read straight from the lattice copy in global memory (neighbouring queries share its lines in L1 / L2): the wide window
// the scattered rest needs, at full lane occupancy, where the tile form would run a 49 x 49 window for one lane in seven.
template <int WR, int CH>
__global__ __launch_bounds__(256) void k_sor_window_list(const float4 *__restrict__ lat, const unsigned int *__restrict__ cell_of, WinGeom g, int mean_k,
                                                          const unsigned int *__restrict__ list, int nq, float *__restrict__ dist, unsigned int *__restrict__ undecided) {
    __shared__ unsigned int s_u[WIN_NB + 1][256];
    const int tid = threadIdx.x, q = blockIdx.x * 256 + tid;
#pragma unroll
    for (int b = 0; b <= WIN_NB; b++) s_u[b][tid] = 0u;
    if (q >= nq) return; // (no workgroup barrier below: the columns are private)
    const unsigned int pt = list[q];
    const unsigned int cell = cell_of[pt]; // the point's lattice position gy * gw + gx
    const float4 *base = lat + (size_t)cell - (size_t)WR * g.gw - WR;
    const float4 P = lat[cell];
    auto ld = [&](int r, int c) { return base[(size_t)r * g.gw + c]; };
    float res = 0.0f;
    double lim = 0.0;
    const bool ok = win_query<WR, CH>(ld, P, g, mean_k, &s_u[0][tid], &res, &lim);
    if (ok) dist[pt] = res;
    undecided[q] = ok ? 0u : 1u; // (indexed like the list: the caller compacts it into the ladder's first list)
}

// What the wave and the workgroup form share per query: the bound and its rounding margin as win_query forms them, the largest squared
// distance h2 that stays below it, the window clipped to the lattice copy (no point lies outside the margin's box) and the squared
// distance to its candidate c < M, row-major.  false: no positive bound -- the query stays undecided.
// (Row and column of candidate c: win_index.h -- a multiplication, exact on its own for windows up to ~1625 pixels a side (M ncx <= 2^32), with one
// correction step beyond; both forms take the split from there, and tests/cpp/win_index_check.cpp and rsm_stage_win_index_check hold it against
// / and % for every candidate of the windows the passes form.)
struct WinCand {
    const float4 *base; // the window's first pixel
    float4 P;
    int gw;             // the lattice copy's row length
    WinIndex ix;        // the window's row length and the constant of the split
    __device__ __forceinline__ float operator()(int c) const { // NaN for a pixel without a point: every comparison fails
        int r, col;
        win_index_split(ix, c, r, col);
        const float4 o = base[(size_t)r * gw + col];
        return fdist2(P.x, P.y, P.z, o.x, o.y, o.z);
    }
};
__device__ __forceinline__ bool win_clip(const float4 *__restrict__ lat, unsigned int cell, const WinGeom &g, int WR, WinCand &cand, float &h2, int &M) {
    const int cy = (int)(cell / (unsigned int)g.gw), cx = (int)(cell - (unsigned int)cy * (unsigned int)g.gw);
    const float4 P = lat[cell];
    const float range = win_bound(P, g, WR).range; // tau must stay below this
    if (!(range > 0.0f && isfinite(range))) return false;
    h2 = __uint_as_float(__float_as_uint(range) - 1u); // d2 <= h2 is d2 < range
    const int x0 = max(cx - WR, 0), x1 = min(cx + WR, g.gw - 1), y0 = max(cy - WR, 0), y1 = min(cy + WR, g.gh - 1);
    cand.ix = win_index_make(x1 - x0 + 1, y1 - y0 + 1); // (M < 2^31: the lattice copy has fewer cells)
    M = cand.ix.ncx * (y1 - y0 + 1);
    cand.base = lat + (size_t)y0 * g.gw + x0;
    cand.P = P;
    cand.gw = g.gw;
    return true;
}

// Wave form: a wave = one listed query -- what the list passes leave: the points within a few dozen pixels of the mask's corners,
// around holes, the outliers this filter exists to remove; hundreds, not millions -- its window of ANY radius read from the lattice
// copy, candidates lane-strided (wave_knn: the grid search's selection).  The same bound as the other forms decides whether
// the window holds the k + 1 nearest (win_clip).
__global__ __launch_bounds__(256) void k_sor_window_wave(const float4 *__restrict__ lat, const unsigned int *__restrict__ cell_of, WinGeom g, int mean_k, int WR,
                                                          const unsigned int *__restrict__ list, int nq, float *__restrict__ dist, unsigned int *__restrict__ undecided) {
    __shared__ float s_d2[4][KNN_CAP];
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return; // wave-uniform; no workgroup barrier below
    const unsigned int pt = list[qi];
    WinCand cand;
    float h2;
    int M;
    if (!win_clip(lat, cell_of[pt], g, WR, cand, h2, M)) {
        if (lane == 0) undecided[qi] = 1u;
        return;
    }
    double sum;
    if (!wave_knn(cand, M, h2, mean_k + 1, s_d2[threadIdx.x >> 6], lane, &undecided[qi], sum)) return;
    if (lane == 0) dist[pt] = (float)(sum / mean_k);
}

// Workgroup form: the wave form's query with its first pass -- every candidate of the window, those within the bound kept -- made by
// four waves together, for the passes that have only hundreds of queries left (C2: 564 at 80 pixels, 15 at 160): a wave per query
// leaves the chip idle and takes as long as its 400 ... 1 600 chunks of candidates do.  Wave w takes the chunks w, w + 4, ... into
// its own quarter of the list (a fixed order: the sum's bits do not depend on timing), the quarters are put together and wave 0
// selects as the wave form does; a quarter that overflows leaves the whole query to wave 0.
__global__ __launch_bounds__(256) void k_sor_window_wg(const float4 *__restrict__ lat, const unsigned int *__restrict__ cell_of, WinGeom g, int mean_k, int WR,
                                                        const unsigned int *__restrict__ list, int nq, float *__restrict__ dist, unsigned int *__restrict__ undecided) {
    constexpr int WG_C = 64, WG_CAP = 64 * WG_C; // (twice the wave form's list: these few queries' windows hold thousands of candidates within the
                                                 // bound, and one pass over them by four waves beats three by one)
    __shared__ float s_seg[4][WG_CAP / 4];
    __shared__ float s_d2[WG_CAP];
    __shared__ int s_cnt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int qi = blockIdx.x;
    const unsigned int pt = list[qi];
    WinCand cand;
    float h2;
    int M;
    if (!win_clip(lat, cell_of[pt], g, WR, cand, h2, M)) { // uniform
        if (threadIdx.x == 0) undecided[qi] = 1u;
        return;
    }
    const int Kw = knn_chunks_list<WG_CAP / 4>(cand, w * 64 * KNN_B, 4 * 64 * KNN_B, M, lane, s_seg[w], [&](float v) { return v <= h2; });
    if (lane == 0) s_cnt[w] = Kw;
    __syncthreads();
    const int k0 = s_cnt[0], k1 = s_cnt[1], k2 = s_cnt[2], k3 = s_cnt[3];
    const bool fits = k0 <= WG_CAP / 4 && k1 <= WG_CAP / 4 && k2 <= WG_CAP / 4 && k3 <= WG_CAP / 4;
    if (fits) {
        const int off = w == 0 ? 0 : (w == 1 ? k0 : (w == 2 ? k0 + k1 : k0 + k1 + k2));
        for (int j = lane; j < Kw; j += 64) s_d2[off + j] = s_seg[w][j];
    }
    __syncthreads();
    if (w != 0) return;
    const int K = fits ? k0 + k1 + k2 + k3 : wave_knn_gather<WG_C>(cand, M, h2, s_d2, lane);
    double sum;
    if (!wave_knn_select<WG_C>(cand, M, h2, mean_k + 1, s_d2, K, lane, &undecided[qi], sum)) return;
    if (lane == 0) dist[pt] = (float)(sum / mean_k);
}

size_t cloud_lattice_bytes(int XL, int XR, int YL, int YR) {
    return sizeof(float4) * (size_t)(XR - XL + 1 + 2 * WIN_PAD) * (size_t)(YR - YL + 1 + 2 * WIN_PAD);
}
WinGeom win_geom(const FilterLattice &L) {
    WinGeom g;
    g.gw = L.XR - L.XL + 1 + 2 * WIN_PAD;
    g.gh = L.YR - L.YL + 1 + 2 * WIN_PAD;
    g.qz = L.qz;
    for (int i = 0; i < 3; i++) {
        g.rz[i] = L.R[3 * i + 2];
        g.T[i] = L.T[i];
    }
    return g;
}
void launch_cloud_lattice(const FilterLattice &L, const WinGeom &g, int64_t n, float4 *lat, unsigned int *cell_of, hipStream_t st) {
    (void)hipMemsetD32Async((hipDeviceptr_t)lat, 0x7fc00000, (size_t)4 * g.gw * g.gh, st);
    hipLaunchKernelGGL(k_cloud_lattice, dim3((unsigned)(L.YR - L.YL + 1)), dim3(256), 0, st, L.flags, L.row_offset, L.W, L.XL, L.XR, L.YL, L.xyz64, n, g.gw, lat,
                       cell_of);
}
void launch_sor_window_list(const float4 *lat, const unsigned int *cell_of, const WinGeom &g, int mean_k, int radius, const unsigned int *list, int nq, float *dist,
                            unsigned int *undecided, hipStream_t st) {
    if (nq <= 0) return;
    if (radius <= 24) hipLaunchKernelGGL((k_sor_window_list<24, 7>), blocks_for(nq), dim3(256), 0, st, lat, cell_of, g, mean_k, list, nq, dist, undecided);
    else hipLaunchKernelGGL((k_sor_window_list<40, 9>), blocks_for(nq), dim3(256), 0, st, lat, cell_of, g, mean_k, list, nq, dist, undecided);
}
void launch_sor_window_wave(const float4 *lat, const unsigned int *cell_of, const WinGeom &g, int mean_k, int radius, const unsigned int *list, int nq, float *dist,
                            unsigned int *undecided, hipStream_t st, int wg_max) {
    if (nq <= 0) return;
    if (nq <= wg_max) // (few enough to leave most of the chip idle at a wave each: four waves per query)
        hipLaunchKernelGGL(k_sor_window_wg, dim3((unsigned)nq), dim3(256), 0, st, lat, cell_of, g, mean_k, radius, list, nq, dist, undecided);
    else
        hipLaunchKernelGGL(k_sor_window_wave, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, lat, cell_of, g, mean_k, radius, list, nq, dist, undecided);
}
void launch_sor_window(const float4 *lat, const WinGeom &g, int mean_k, int radius, float *dist, unsigned int *undecided, hipStream_t st, int tile_step,
                       unsigned int *probe_cnt) {
    const int tx = (g.gw - 2 * WIN_PAD + WIN_TX - 1) / WIN_TX, ty = (g.gh - 2 * WIN_PAD + WIN_TY - 1) / WIN_TY; // tiles over the margin's box
    const dim3 grid((unsigned)((tx + tile_step - 1) / tile_step), (unsigned)((ty + tile_step - 1) / tile_step));
#define WIN_LAUNCH(R_)                                                                                                                     \
    do {                                                                                                                                   \
        if (probe_cnt) hipLaunchKernelGGL((k_sor_window<R_, true>), grid, dim3(256), 0, st, lat, g, mean_k, dist, undecided, tile_step, probe_cnt); \
        else hipLaunchKernelGGL((k_sor_window<R_, false>), grid, dim3(256), 0, st, lat, g, mean_k, dist, undecided, tile_step, probe_cnt);          \
    } while (0)
    switch (radius) {
    case 7: WIN_LAUNCH(7); break;
    case 12: WIN_LAUNCH(12); break;
    case 16: WIN_LAUNCH(16); break;
    case 20: WIN_LAUNCH(20); break;
    default: WIN_LAUNCH(24); break;
    }
#undef WIN_LAUNCH
}
