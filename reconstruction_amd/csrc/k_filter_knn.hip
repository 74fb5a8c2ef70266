// k_filter_knn.hip -- the cloud filter's k-nearest searches off the pixel lattice (k_filter.hip's head comment: "Neighbour search"; the host
// steps that run them are there): a grid level's 27 cells a wave per query (k_sor_knn), and what no level decides against ALL points (k_xq_*).
#include "filter_units.h"
#include "knn_select.h"

#include <algorithm>

__device__ __forceinline__ float3 load_point(const float *__restrict__ xyz, unsigned int i) { // a query's own coordinates
    return make_float3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
}
__device__ __forceinline__ int lower_bound_key_in(const unsigned long long *__restrict__ keys, int lo, int hi, unsigned long long k) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// mean distance to the k nearest neighbours (statistical_outlier_removal.hpp).  One wave per query point: the 27 cells
// around it are 9 contiguous ranges of the sorted array -- their ends come from the cell table (lanes 0..26 load one
// cell each: one round trip) or, without a table, from binary searches; the squared distances to the candidates are
// computed once into registers (lane l holds candidates l, l + 64, ...; the asm fence keeps the compiler from
// re-loading them in every bisection step -- the first version did, 36 VGPRs and 120 ns per query), the (k+1)-th
// smallest is found by bisection on its bit pattern with ballots, the sum by a wave reduction.
// A query with more than 64 * KNN_C candidates re-computes them per bisection step instead.
template <int TABLE> // 1: per-cell table, 2: per-row table + a short binary search inside the row, 0: binary search on all keys
__global__ __launch_bounds__(256) void k_sor_knn(const float *__restrict__ xyz, const float4 *__restrict__ sxyz,
                                                  const unsigned long long *__restrict__ keys, const int2 *__restrict__ table, int n,
                                                  FGrid g, float h2, int mean_k, const unsigned int *__restrict__ queries, int nq,
                                                  float *__restrict__ dist_orig, unsigned int *__restrict__ undecided /* [nq]: 1 = retry on a coarser grid */) {
    __shared__ float s_d2[4][KNN_CAP];
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return; // wave-uniform; no workgroup barrier below
    const unsigned int orig = queries[qi];
    const float3 p = load_point(xyz, orig);
    int ix, iy, iz;
    grid_cell(g, p.x, p.y, p.z, ix, iy, iz);
    int my_s = 0, my_e = 0; // range t in lane t (t < 9)
    if (TABLE == 2) {
        if (lane < 9) {
            const int yy = iy + lane % 3 - 1, zz = iz + lane / 3 - 1;
            if (yy >= 0 && yy < g.ny && zz >= 0 && zz < g.nz) {
                const unsigned long long row = (unsigned long long)zz * g.ny + yy, base = row * g.nx;
                const int2 se = table[row];
                my_s = lower_bound_key_in(keys, se.x, se.y, base + max(ix - 1, 0));
                my_e = lower_bound_key_in(keys, my_s, se.y, base + min(ix + 1, g.nx - 1) + 1);
            }
        }
    } else if (TABLE == 1) {
        // lane 3 t + j: cell (ix - 1 + j, iy + t % 3 - 1, iz + t / 3 - 1); its points are [x, y) of the sorted array
        int cs = 0, ce = 0;
        if (lane < 27) {
            const int t = lane / 3, xx = ix - 1 + lane % 3, yy = iy + t % 3 - 1, zz = iz + t / 3 - 1;
            if (xx >= 0 && xx < g.nx && yy >= 0 && yy < g.ny && zz >= 0 && zz < g.nz) {
                const int2 se = table[((size_t)zz * g.ny + yy) * g.nx + xx];
                cs = se.x;
                ce = se.y;
            }
        }
        // the three x-adjacent cells hold consecutive keys: first non-empty cell's start .. last non-empty cell's end
        const int s0 = __shfl(cs, 3 * lane), s1 = __shfl(cs, 3 * lane + 1), s2 = __shfl(cs, 3 * lane + 2);
        const int e0 = __shfl(ce, 3 * lane), e1 = __shfl(ce, 3 * lane + 1), e2 = __shfl(ce, 3 * lane + 2);
        if (lane < 9) {
            my_s = e0 > s0 ? s0 : (e1 > s1 ? s1 : s2);
            my_e = e2 > s2 ? e2 : (e1 > s1 ? e1 : (e0 > s0 ? e0 : my_s));
            if (!(e0 > s0 || e1 > s1 || e2 > s2)) my_s = my_e = 0;
        }
    } else if (lane < 9) {
        const int yy = iy + lane % 3 - 1, zz = iz + lane / 3 - 1;
        if (yy >= 0 && yy < g.ny && zz >= 0 && zz < g.nz) {
            const unsigned long long base = ((unsigned long long)zz * g.ny + yy) * g.nx;
            my_s = lower_bound_key(keys, n, base + max(ix - 1, 0));
            my_e = lower_bound_key(keys, n, base + min(ix + 1, g.nx - 1) + 1);
        }
    }
    int rs[9], pre[10];
    pre[0] = 0;
#pragma unroll
    for (int t = 0; t < 9; t++) {
        rs[t] = __shfl(my_s, t);
        pre[t + 1] = pre[t] + (__shfl(my_e, t) - rs[t]);
    }
    const int M = pre[9], want = mean_k + 1; // the point itself is the first of the k + 1 results
    auto cand = [&](int c) -> float { // squared distance to candidate c < M of the concatenated ranges
        int base = rs[0] - pre[0];
#pragma unroll
        for (int t = 1; t < 9; t++) base = c >= pre[t] ? rs[t] - pre[t] : base;
        const float4 o = sxyz[base + c];
        return fdist2(p.x, p.y, p.z, o.x, o.y, o.z);
    };
    double sum;
    if (!wave_knn(cand, M, h2, want, s_d2[threadIdx.x >> 6], lane, &undecided[qi], sum)) return;
    if (lane == 0) dist_orig[orig] = (float)(sum / mean_k);
}

// ---- the few queries no grid level could decide (isolated points -- what this filter removes -- and clusters smaller
// than k): against ALL points, the whole chip on every query.  Three-pass radix select of the (k+1)-th smallest squared
// distance (bits 30..20, 19..9, 8..0 of its pattern): per pass every workgroup histograms its slice of the points for
// one query and adds the non-empty bins to the query's global histogram, a one-workgroup kernel picks the bin; then the
// slices' partial sums of sqrt(d2) over d2 < tau are added up as the workgroups retire -- PCL's bits only if no addition rounded:
// k_xq_finish tests that (knn_sum_exact) and adds a query that fails it again, sequentially and ascending.
#define XQ_SLICES 128
#define XQ_LIST 4096 // values below tau a workgroup of k_xq_finish lists in LDS (more: it re-reads the points per distinct value)
__device__ __forceinline__ int2 xq_slice(int n) { // the points [x, y) of n that workgroup blockIdx.x of the XQ_SLICES takes
    const int per = (n + XQ_SLICES - 1) / XQ_SLICES, q0 = blockIdx.x * per;
    return make_int2(q0, min(n, q0 + per));
}
__global__ void k_xq_init(XqState *__restrict__ st, int count, int mean_k, int n) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= count) return;
    st[q].prefix = 0u;
    st[q].mask = 0u;
    st[q].rank = min(mean_k + 1, n);
    st[q].less = 0;
    st[q].sum = 0.0;
    st[q].min_m1 = 0xffffffffu;
}
__global__ __launch_bounds__(256) void k_xq_hist(const float *__restrict__ xyz, const float4 *__restrict__ sxyz, int n,
                                                  const unsigned int *__restrict__ list, int count,
                                                  const XqState *__restrict__ st, int shift, int width, int *__restrict__ ghist) {
    __shared__ int hist[2048];
    const int2 slice = xq_slice(n);
    for (int item = blockIdx.y; item < count; item += gridDim.y) { // uniform
        const unsigned int orig = list[item];
        const float3 p = load_point(xyz, orig);
        const unsigned int prefix = st[item].prefix, mask = st[item].mask;
        for (int b = threadIdx.x; b < 2048; b += 256) hist[b] = 0;
        __syncthreads();
        for (int q = slice.x + threadIdx.x; q < slice.y; q += 256) {
            const float4 o = sxyz[q];
            const unsigned int u = __float_as_uint(fdist2(p.x, p.y, p.z, o.x, o.y, o.z));
            // the distances to one far query share a handful of bins: one LDS atomic per distinct bin of the wave
            int bin = ((u & mask) == prefix) ? (int)((u >> shift) & ((1u << width) - 1u)) : -1;
            while (__ballot(bin >= 0)) { // uniform
                const unsigned long long act = __ballot(bin >= 0);
                const int b0 = __shfl(bin, __ffsll((long long)act) - 1);
                const unsigned long long same = __ballot(bin == b0);
                if (((int)threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(&hist[b0], __popcll(same));
                if (bin == b0) bin = -1;
            }
        }
        __syncthreads();
        for (int b = threadIdx.x; b < (1 << width); b += 256)
            if (hist[b]) atomicAdd(&ghist[(size_t)item * 2048 + b], hist[b]);
        __syncthreads();
    }
}
__global__ __launch_bounds__(64) void k_xq_pick(XqState *__restrict__ st, int count, int shift, int width,
                                                 int *__restrict__ ghist) {
    const int item = blockIdx.x;
    if (item >= count) return;
    int *h = ghist + (size_t)item * 2048;
    if (threadIdx.x == 0) {
        int rank = st[item].rank, b = 0;
        for (; b < (1 << width) - 1; b++) {
            if (h[b] >= rank) break;
            rank -= h[b];
        }
        st[item].rank = rank;
        st[item].prefix |= (unsigned int)b << shift;
        st[item].mask |= ((1u << width) - 1u) << shift;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 2048; b += 64) h[b] = 0; // ready for the next pass
}
__global__ __launch_bounds__(256) void k_xq_sum(const float *__restrict__ xyz, const float4 *__restrict__ sxyz, int n,
                                                 const unsigned int *__restrict__ list, int count,
                                                 XqState *__restrict__ st) {
    __shared__ double s_sum[4];
    __shared__ int s_less[4];
    __shared__ unsigned int s_min[4];
    const int2 slice = xq_slice(n);
    for (int item = blockIdx.y; item < count; item += gridDim.y) {
        const unsigned int orig = list[item];
        const float3 p = load_point(xyz, orig);
        const float tau = __uint_as_float(st[item].prefix);
        double sum = 0.0;
        int less = 0;
        unsigned int min_m1 = 0xffffffffu;
        for (int q = slice.x + threadIdx.x; q < slice.y; q += 256) {
            const float4 o = sxyz[q];
            const float d2 = fdist2(p.x, p.y, p.z, o.x, o.y, o.z);
            if (d2 < tau) {
                sum += (double)sqrtf(d2);
                less++;
                min_m1 = knn_min_m1(min_m1, d2);
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o);
            less += __shfl_xor(less, o);
            min_m1 = min(min_m1, (unsigned int)__shfl_xor((int)min_m1, o));
        }
        if ((threadIdx.x & 63) == 0) {
            s_sum[threadIdx.x >> 6] = sum;
            s_less[threadIdx.x >> 6] = less;
            s_min[threadIdx.x >> 6] = min_m1;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int l = s_less[0] + s_less[1] + s_less[2] + s_less[3];
            if (l) { // (the order of these additions is the workgroups': k_xq_finish accepts the sum only if none of them can have rounded)
                atomicAdd(&st[item].sum, (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));
                atomicAdd(&st[item].less, l);
                atomicMin(&st[item].min_m1, min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3])));
            }
        }
        __syncthreads();
    }
}
// A workgroup per listed query: the mean distance from the slices' sum, or -- its order mattered -- from the sequential ascending sum
// over the values below tau: listed in LDS by one more pass over the points (at most k of them), else read again per distinct value.
__global__ __launch_bounds__(256) void k_xq_finish(const float *__restrict__ xyz, const float4 *__restrict__ sxyz, int n_arr, const XqState *__restrict__ st,
                                                    const unsigned int *__restrict__ list, int count, int mean_k, int n, float *__restrict__ dist_orig) {
    __shared__ unsigned int s_v[XQ_LIST];
    __shared__ int s_m[4], s_c[4], s_n;
    const int item = blockIdx.x; // (< count: the grid)
    const int want = min(mean_k + 1, n), less = st[item].less;
    const float tau = __uint_as_float(st[item].prefix);
    const unsigned int orig = list[item];
    double sum = st[item].sum + (double)(want - less) * (double)sqrtf(tau);
    if (__builtin_expect(!knn_sum_exact(sum, knn_min_m1(st[item].min_m1, tau)), 0)) { // uniform
        const float3 p = load_point(xyz, orig);
        const bool listed = less <= XQ_LIST;
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        if (listed) {
            for (int q = threadIdx.x; q < n_arr; q += 256) {
                const float4 o = sxyz[q];
                const float d2 = fdist2(p.x, p.y, p.z, o.x, o.y, o.z);
                if (d2 < tau && d2 > 0.0f) s_v[min(atomicAdd(&s_n, 1), XQ_LIST - 1)] = __float_as_uint(d2); // (at most less <= XQ_LIST of them)
            }
            __syncthreads();
        }
        const int nl = min(s_n, XQ_LIST);
        sum = knn_sum_ascending(
            [&](unsigned int from, unsigned int &m, int &cnt) { // every thread gets the workgroup's m and cnt
                auto each = [&](auto &&f) {
                    if (listed) {
                        for (int j = threadIdx.x; j < nl; j += 256) f(s_v[j]);
                    } else {
                        for (int q = threadIdx.x; q < n_arr; q += 256) {
                            const float4 o = sxyz[q];
                            f(__float_as_uint(fdist2(p.x, p.y, p.z, o.x, o.y, o.z)));
                        }
                    }
                };
                auto reduce = [&](auto &v, auto *s, auto &&op) { // over the workgroup, into every thread
                    v = wave_reduce(v, op);
                    __syncthreads();
                    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
                    __syncthreads();
                    v = op(op(s[0], s[1]), op(s[2], s[3]));
                };
                int mi = (int)(m ^ 0x80000000u); // (shuffled and compared as int: the sign bit flipped keeps the unsigned order)
                each([&](unsigned int u) { mi = (u >= from) ? min(mi, (int)(u ^ 0x80000000u)) : mi; });
                reduce(mi, s_m, [](int a, int b) { return min(a, b); });
                m = (unsigned int)mi ^ 0x80000000u;
                cnt = 0;
                each([&](unsigned int u) { cnt += u == m; });
                reduce(cnt, s_c, [](int a, int b) { return a + b; });
            },
            tau, want - less);
    }
    if (threadIdx.x == 0) dist_orig[orig] = (float)(sum / mean_k);
}

void launch_knn(const float *d_xyz, const FilterGridDev &G, int nv, float h, int mean_k, const unsigned int *queries, int nq, float *d_dist,
                unsigned int *d_cnt /* undecided flags */, hipStream_t st) {
    const dim3 grid((unsigned)((nq + 3) / 4));
    if (G.table_kind == 1)
        hipLaunchKernelGGL(k_sor_knn<1>, grid, dim3(256), 0, st, d_xyz, G.sxyz, G.keys, G.table, nv, G.g, h * h, mean_k, queries, nq, d_dist, d_cnt);
    else if (G.table_kind == 2)
        hipLaunchKernelGGL(k_sor_knn<2>, grid, dim3(256), 0, st, d_xyz, G.sxyz, G.keys, G.table, nv, G.g, h * h, mean_k, queries, nq, d_dist, d_cnt);
    else
        hipLaunchKernelGGL(k_sor_knn<0>, grid, dim3(256), 0, st, d_xyz, G.sxyz, G.keys, G.table, nv, G.g, h * h, mean_k, queries, nq, d_dist, d_cnt);
}
void launch_xq_search(const float *d_xyz, const float4 *arr, int arr_n, const unsigned int *list, int cnt, XqState *d_xq, int *d_hist, int mean_k, int nv,
                      float *d_dist, hipStream_t st) {
    const int shifts[3] = {20, 9, 0}, widths[3] = {11, 11, 9};
    const int qy = std::min(cnt, 1024);
    hipLaunchKernelGGL(k_xq_init, blocks_for(cnt), dim3(256), 0, st, d_xq, cnt, mean_k, nv);
    for (int pass = 0; pass < 3; pass++) {
        hipLaunchKernelGGL(k_xq_hist, dim3(XQ_SLICES, (unsigned)qy), dim3(256), 0, st, d_xyz, arr, arr_n, list, cnt, d_xq, shifts[pass], widths[pass], d_hist);
        hipLaunchKernelGGL(k_xq_pick, dim3((unsigned)cnt), dim3(64), 0, st, d_xq, cnt, shifts[pass], widths[pass], d_hist);
    }
    hipLaunchKernelGGL(k_xq_sum, dim3(XQ_SLICES, (unsigned)qy), dim3(256), 0, st, d_xyz, arr, arr_n, list, cnt, d_xq);
    hipLaunchKernelGGL(k_xq_finish, dim3((unsigned)cnt), dim3(256), 0, st, d_xyz, arr, arr_n, d_xq, list, cnt, mean_k, nv, d_dist);
}
