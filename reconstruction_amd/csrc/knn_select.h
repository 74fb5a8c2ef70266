// knn_select.h -- what the cloud filter's k-nearest searches (k_filter_win.hip: the pixel windows, k_filter_knn.hip: the grid cells and the whole
// cloud) share on the device: the square root and the exact-sum rules of the k-nearest sums, and the selection a wave runs
// for one query -- gather the candidates within the bound into a list, select among the listed.
#pragma once

#include "wave_prims.h" // wave_reduce / wave_sum / wave_min / wave_max

// sqrtf, correctly rounded, for the k-nearest sums (PCL adds sqrt of the float32 squared distances): the compiler's own sequence --
// v_sqrt_f32 (1 ulp), the two neighbouring floats, an fma residual each, two selects -- WITHOUT its input scaling for
// denormals and its zero / infinity test (8 of 17 instructions): the same bits for every x in [2^-96, FLT_MAX] and for 0
// (rsm_stage_sqrt_check holds it against sqrtf on ALL of them); anything else takes sqrtf.  The pixel-window search spends its
// second pass in this function with a tenth of its lanes active.
__device__ __forceinline__ float sqrtf_rn_core(float x) { // x in [2^-96, FLT_MAX] or 0
    float s = __builtin_amdgcn_sqrtf(x);
    const float s_dn = __uint_as_float(__float_as_uint(s) - 1u), s_up = __uint_as_float(__float_as_uint(s) + 1u);
    const float r_dn = __builtin_fmaf(-s_dn, s, x), r_up = __builtin_fmaf(-s_up, s, x);
    s = (r_dn <= 0.0f) ? s_dn : s;
    s = (r_up > 0.0f) ? s_up : s;
    return s;
}
__device__ __forceinline__ float sqrtf_rn(float x) {
    if (__builtin_expect(!(x >= 0x1p-96f || x == 0.0f), 0)) return sqrtf(x); // denormal-range inputs (and NaN / negative): the general sequence
    return sqrtf_rn_core(x);
}

// ---- the k-nearest sum's order.  PCL (and oracle/cloud_oracle.c) add sqrtf of the k nearest squared distances into a double one after the
// other, ascending.  Any other order gives the same bits as long as no addition rounds: the values are non-negative float32, each a
// multiple of 2^q with q = (exponent of the smallest positive one) - 23, so every partial sum is a multiple of 2^q, and one below
// 2^(q + 53) is representable.  min_m1 = the smallest positive SQUARED distance's bit pattern minus one (0xffffffff: none -- zeros add
// exactly), total = the whole sum as the parallel order gave it (+inf / NaN fail the test).
__device__ __forceinline__ unsigned int knn_min_m1(unsigned int min_m1, float d2) { return min(min_m1, __float_as_uint(d2) - 1u); } // (0 wraps to the top)
__device__ __forceinline__ bool knn_sum_exact(double total, unsigned int min_m1) {
    if (min_m1 == 0xffffffffu) return true;
    const int e = (int)(__float_as_uint(sqrtf(__uint_as_float(min_m1 + 1u))) >> 23); // biased; the root of a positive float32 is a normal one
    return total < __hiloint2double((e - 150 + 53 + 1023) << 20, 0);                // 2^(q + 53), q = e - 127 - 23
}
// The sum in PCL's order, for the queries that fail the test.  next(from, m, cnt): m = the smallest squared distance's bit pattern in
// [from, tau) among the query's candidates, cnt = how many carry it; m >= tau's pattern: none is left (wave- or workgroup-uniform).  Equal
// values are interchangeable, so the order among them is no choice; `ties` values equal tau itself close the sum.
template <class Next>
__device__ __forceinline__ double knn_sum_ascending(const Next &next, float tau, int ties) {
    const unsigned int tau_b = __float_as_uint(tau);
    double s = 0.0;
    for (unsigned int from = 1u; from < tau_b;) { // (zeros add nothing)
        unsigned int m = tau_b;
        int cnt = 0;
        next(from, m, cnt);
        if (m >= tau_b) break;
        const double v = (double)sqrtf(__uint_as_float(m));
        for (int c = 0; c < cnt; c++) s += v;
        from = m + 1u;
    }
    const double vt = (double)sqrtf(tau);
    for (int c = 0; c < ties; c++) s += vt;
    return s;
}

#define KNN_C 32    // registers per lane for the candidates within h
#define KNN_CAP (64 * KNN_C)
#define KNN_B 16    // candidate loads in flight per lane
// The selection a wave runs for one query over M candidates `cand(c)` (squared float32 distances, NaN = no candidate): the (k+1)-th
// smallest among those <= h2 and the sum of the `want` smallest square roots (the query's own 0 among them) as PCL's sequential
// ascending loop forms it.  Shared by the grid search (k_sor_knn: the 27 cells of a query) and the wave and workgroup forms of the
// pixel-window search (k_sor_window_wave / k_sor_window_wg: a window of the lattice copy).  Two jobs: wave_knn_gather lists the
// candidates within h2, wave_knn_select selects among the listed; wave_knn is the one after the other.

// The chunked candidate pass: a wave over the chunks first, first + stride, ... of the M candidates -- KNN_B loads per lane in flight,
// then each(v) per value in a fixed order (candidate c0 + lane + 64 i; +inf past the last).
template <class Cand, class Each>
__device__ __forceinline__ void knn_chunks(const Cand &cand, int first, int stride, int M, int lane, const Each &each) {
    const float inf = __uint_as_float(0x7f800000u);
    for (int c0 = first; c0 < M; c0 += stride) { // uniform
        float v[KNN_B];
#pragma unroll
        for (int i = 0; i < KNN_B; i++) {
            const int c = c0 + lane + 64 * i;
            v[i] = (c < M) ? cand(c) : inf;
        }
#pragma unroll
        for (int i = 0; i < KNN_B; i++) each(v[i]);
    }
}
// ... with those that keep(v) accepts compacted into `list` by ballot and popcount (the first CAP of them, in the pass's order);
// returns how many there are (uniform)
template <int CAP, class Cand, class Keep>
__device__ __forceinline__ int knn_chunks_list(const Cand &cand, int first, int stride, int M, int lane, float *list, const Keep &keep_of) {
    const unsigned long long lt = (1ull << lane) - 1ull;
    int K = 0;
    knn_chunks(cand, first, stride, M, lane, [&](float v) {
        const bool keep = keep_of(v);
        const unsigned long long mm = __ballot(keep);
        const int pos = K + __popcll(mm & lt);
        if (keep && pos < CAP) list[pos] = v;
        K += __popcll(mm);
    });
    return K;
}

// Only candidates within h of the query matter (a query is decided here iff k + 1 of them exist): the squared
// distances are computed in chunks of KNN_B loads per lane in flight, those <= h^2 are compacted into the wave's
// LDS list (about a third of the 27 cells' points for a surface, a sixth for a volume) and read back into registers,
// lane l holding entries l, l + 64, ...; the asm fence keeps the compiler from re-deriving them from memory in
// every bisection step (the first version did: 120 ns per query).
// Returns K, the candidates within h2 (uniform); `mine` holds the first 64 C_ of them.
template <int C_ = KNN_C, class Cand>
__device__ __forceinline__ int wave_knn_gather(const Cand &cand, int M, float h2, float *mine, int lane) {
    return knn_chunks_list<64 * C_>(cand, 0, 64 * KNN_B, M, lane, mine, [&](float v) { return v <= h2; });
}

// Among the K candidates within h2, of which `mine` holds the first 64 C_ in a fixed order.  Returns false -- nothing written but
// `undecided` -- when fewer than `want` candidates lie within h2 (or the sum's order matters and the list that would order it has
// overflowed).
template <int C_ = KNN_C, class Cand>
__device__ __forceinline__ bool wave_knn_select(const Cand &cand, int M, float h2, int want, float *mine, int K, int lane, unsigned int *undecided_slot,
                                                double &sum_out) {
    constexpr int CAP_ = 64 * C_; // the list's capacity: C_ registers per lane in the selection
    const float inf = __uint_as_float(0x7f800000u);
    // (a flag per query, compacted by a scan afterwards: appending to one list through a single counter retires ~88
    // appends per microsecond -- 62 ms for a level that decides nothing)
    if (lane == 0) *undecided_slot = K < want;
    if (K < want) return false; // not decidable among these candidates
    if (K > CAP_ && h2 > 0.0f) {
        // More candidates within h than the list holds (a wide window over a dense part, a too-coarse grid level): two more passes
        // narrow them down instead of a 30-step bisection that re-reads them all in every step -- a histogram of the squared
        // distances over CAP_ equal bins of [0, h2] (the list's LDS), the bin b* holding rank `want`, then the list again with
        // the candidates of bins <= b* only (bin() is monotone: they are exactly the values up to some threshold, the rank's among
        // them).  Falls through to the bisection only if even that is too many (thousands of equal distances).
        int *hist = (int *)mine;
        const float inv_w = (float)CAP_ / h2;
        auto bin_of = [&](float v) { return min((int)(v * inv_w), CAP_ - 1); };
        if (isfinite(inv_w) && inv_w > 0.0f) {
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int i = 0; i < C_; i++) hist[lane + 64 * i] = 0;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            knn_chunks(cand, 0, 64 * KNN_B, M, lane, [&](float v) {
                if (v <= h2) atomicAdd(&hist[bin_of(v)], 1);
            });
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // lane l owns bins [32 l, 32 l + 32): its total, the wave's exclusive prefix, then the bin inside the owning lane
            int mine_sum = 0;
#pragma unroll
            for (int i = 0; i < C_; i++) mine_sum += hist[lane * C_ + i];
            int incl = mine_sum;
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            const unsigned long long has = __ballot(incl >= want);
            const int owner = __builtin_ctzll(has); // (K >= want: some lane reaches it)
            int run = __shfl(incl - mine_sum, owner), bstar = owner * C_, upto = 0;
            for (int i = 0; i < C_; i++) { // uniform: every lane reads the owner's bins
                const int hcount = hist[owner * C_ + i];
                run += hcount;
                if (run >= want) {
                    bstar = owner * C_ + i;
                    upto = run;
                    break;
                }
            }
            if (upto >= want && upto <= CAP_) {
                __builtin_amdgcn_wave_barrier();
                K = knn_chunks_list<CAP_>(cand, 0, 64 * KNN_B, M, lane, mine, [&](float v) { return v <= h2 && bin_of(v) <= bstar; });
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            } else {
                K = CAP_ + 1; // (the list's LDS holds the histogram now: the bisection below reads the candidates themselves)
            }
        }
    }
    float tau;
    double sum = 0.0;
    int less = 0;
    unsigned int min_m1 = 0xffffffffu; // (knn_sum_exact)
    if (K <= CAP_) {
        __builtin_amdgcn_wave_barrier();
        float d2[C_];
        const int nreg = (K + 63) >> 6; // wave-uniform
#pragma unroll
        for (int i = 0; i < C_; i++) {
            d2[i] = inf;
            if (i < nreg && lane + 64 * i < K) d2[i] = mine[lane + 64 * i];
        }
#pragma unroll
        for (int i = 0; i < C_; i++) asm volatile("" : "+v"(d2[i])); // materialise: the values live in registers from here on (the fences AFTER
                                                                        // the last read: one right behind each read makes it a round trip of its own)
        auto count4 = [&](float t, int i0) {
            int cnt = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) cnt += __popcll(__ballot(d2[i0 + i] <= t));
            return cnt;
        };
        auto count_le = [&](float t) { // registers past nreg hold +inf; whole groups of 4 are skipped (uniform)
            int cnt = count4(t, 0);
#pragma unroll
            for (int g4 = 1; g4 < C_ / 4; g4++)
                if (nreg > 4 * g4) cnt += count4(t, 4 * g4);
            return cnt;
        };
        // smallest bit pattern b with count_le(b) >= want = the want-th smallest value.  A step that counts EXACTLY want
        // has it bracketed -- it is the largest value <= mid -- which happens after ~log2(K) of the 30 steps unless equal
        // distances straddle the rank (then the bisection runs to the end as before).  (Snapping the bracket to the data
        // in every step -- a wave min / max reduction per step, ~9 steps -- measured slower: 46 instead of 39.5 ms.)
        unsigned int lo = 0u, hi = __float_as_uint(h2);
        while (lo < hi) {
            const unsigned int mid = lo + ((hi - lo) >> 1);
            const int cnt = count_le(__uint_as_float(mid));
            if (cnt == want) {
                const float fm = __uint_as_float(mid);
                float m = 0.0f;
#pragma unroll
                for (int i = 0; i < C_; i++)
                    if (i < nreg && d2[i] <= fm) m = fmaxf(m, d2[i]);
                lo = hi = __float_as_uint(wave_max(m));
                break;
            }
            if (cnt >= want) hi = mid;
            else lo = mid + 1;
        }
        tau = __uint_as_float(lo);
#pragma unroll
        for (int i = 0; i < C_; i++)
            if (i < nreg && d2[i] < tau) {
                sum += (double)sqrtf(d2[i]);
                less++;
                min_m1 = knn_min_m1(min_m1, d2[i]);
            }
    } else { // more than CAP_ points within h (a far too coarse first level): bisection straight on the candidates
        auto count_le = [&](float t) {
            int cnt = 0;
            for (int c0 = 0; c0 < M; c0 += 64) { // uniform trip count
                const int c = c0 + lane;
                cnt += __popcll(__ballot(c < M && cand(min(c, M - 1)) <= t));
            }
            return cnt;
        };
        unsigned int lo = 0u, hi = __float_as_uint(h2);
        while (lo < hi) {
            const unsigned int mid = lo + ((hi - lo) >> 1);
            if (count_le(__uint_as_float(mid)) >= want) hi = mid;
            else lo = mid + 1;
        }
        tau = __uint_as_float(lo);
        for (int c = lane; c < M; c += 64) {
            const float v = cand(c);
            if (v < tau) {
                sum += (double)sqrtf(v);
                less++;
                min_m1 = knn_min_m1(min_m1, v);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { // (three values a step: wave_sum / wave_min one after the other order the instructions differently)
        sum += __shfl_xor(sum, o);
        less += __shfl_xor(less, o);
        min_m1 = min(min_m1, (unsigned int)__shfl_xor((int)min_m1, o));
    }
    sum += (double)(want - less) * (double)sqrtf(tau); // the values equal to tau that the rank takes in
    if (__builtin_expect(!knn_sum_exact(sum, knn_min_m1(min_m1, tau)), 0)) { // the order matters: PCL's
        if (K > CAP_) { // (no list to add from: the query is left to the passes behind this one; the whole-cloud search at the end lists)
            if (lane == 0) *undecided_slot = 1u;
            return false;
        }
        sum = knn_sum_ascending(
            [&](unsigned int from, unsigned int &m, int &cnt) { // (the list is still what the registers were read from)
                for (int j = lane; j < K; j += 64) m = (__float_as_uint(mine[j]) >= from) ? min(m, __float_as_uint(mine[j])) : m;
                m = wave_min(m);
                for (int j = lane; j < K; j += 64) cnt += __float_as_uint(mine[j]) == m;
                cnt = wave_sum(cnt);
            },
            tau, want - less);
    }
    sum_out = sum;
    return true;
}

// gather, then select: the wave's whole job for a query whose candidates no one has listed yet
template <int C_ = KNN_C, class Cand>
__device__ __forceinline__ bool wave_knn(const Cand &cand, int M, float h2, int want, float *mine, int lane, unsigned int *undecided_slot, double &sum_out) {
    if (M < want) { // fewer points in the 27 cells than neighbours wanted: undecidable without looking at them
        if (lane == 0) *undecided_slot = 1u;
        return false;
    }
    return wave_knn_select<C_>(cand, M, h2, want, mine, wave_knn_gather<C_>(cand, M, h2, mine, lane), lane, undecided_slot, sum_out);
}
