// k_filter.hip -- the per-pair cloud filter of CCloudOptimization::filter (CloudOptimization/CCloudOptimization.cpp:82-121),
// SURVEY 8(f3), on the GPU that produced the cloud (it runs before the RCCL gather and shrinks its payload):
//   pcl::StatisticalOutlierRemoval, meanK = 100, stddevMulThresh = 1 (:85-89; parameters CReconstruction.cpp:18)
//   pcl::NormalEstimationOMP, radius search m_mls_radius = 2.5 (:103-109)
//   normals turned toward CamCenter (:114-121)
// PCL is a third-party dependency that is not in the reference tree; the algorithms are restated from PCL 1.7.2's
// published sources exactly as oracle/cloud_oracle.c states them (parity unpinned; same documented choices: float32
// neighbour distances, dist^2 < r^2, double accumulators).
//
// Neighbour search: the points are sorted by the key of a uniform grid (cell edge h); the 3 x-adjacent cells of one
// (y, z) row of cells have consecutive keys, so the 27 cells around a point are 9 contiguous ranges of the sorted
// array, found by binary search on the keys (no hash table).  Threads walk the sorted order, so the lanes of a wave
// search the same few ranges and their loads coalesce.
//   k nearest: every point within distance h of p lies in those 27 cells.  The (k+1)-th smallest squared distance tau
//     (the point itself included, as in PCL's nearestKSearch(k + 1)) is found by bisection on its float bit pattern over
//     [0, h^2], re-scanning the candidates per step (~900 candidates from L1/L2: cheaper than keeping 100 running minima
//     per thread); then sum sqrt(d2) over d2 < tau + (k + 1 - #less) sqrt(tau).  PCL adds these float32 values into a double one
//     after the other, ascending.  The lanes add them in another order, which gives the same bits only while no addition rounds:
//     knn_sum_exact tests that per query (every value a multiple of 2^q, the total below 2^(q + 53)) and a query that fails it --
//     a near-duplicate beside neighbours 2^22 times as far -- gets the sequential ascending sum (knn_sum_ascending).
//     Points with fewer than k + 1 candidates within h (isolated points -- what this filter removes -- and patch
//     corners) go to a list and are redone against ALL points by a workgroup each (three-pass radix select).
//   radius search: cell edge = radius, the 27 cells cover the ball.
// A cloud that is the depth map of a matched pair is searched on its pixel lattice first; the grids see what that leaves.
// This unit: the host steps (FilterRun, filter_cloud_device), the per-point kernels and the normals.  The k-nearest searches are units of
// their own, reached through filter_units.h's launchers: k_filter_win.hip (the pixel windows) and k_filter_knn.hip (the grid cells, the
// whole cloud); what they share on the device is knn_select.h (the selection, the exact-sum rules), and win_bound.h with the normals here.
// Between the outlier removal and the normals sits, when the caller switches it on (FilterRoute::outrem), the radius outlier pass of :90-96
// (pcl::RadiusOutlierRemoval, commented out in the shipped reference): its kernels and its definition are k_filter_outrem.hip's, its host
// step is outrem_pass here.
#include "../../include/rsm.h"
#include "filter_units.h"
#include "knn_select.h"
#include "win_index.h"

#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

// test entry (rsm_stage_sqrt_check): sqrtf_rn against sqrtf on the floats with bit patterns first .. first + n - 1
__global__ void k_sqrt_check(unsigned int first, long long n, unsigned long long *mismatches) {
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    unsigned int bad = 0;
    for (long long i = i0; i < n; i += stride) {
        const float x = __uint_as_float(first + (unsigned int)i);
        bad += __float_as_uint(sqrtf_rn(x)) != __float_as_uint(sqrtf(x));
    }
    if (bad) atomicAdd(mismatches, (unsigned long long)bad);
}
void launch_sqrt_check(unsigned int first, long long n, unsigned long long *mismatches, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_sqrt_check, dim3(8192), dim3(256), 0, st, first, n, mismatches);
}
// test entry (rsm_stage_win_index_check): win_index.h's split against the device's own c / ncx and c % ncx on every candidate of an
// ncx x ncy window
__global__ void k_win_index_check(WinIndex w, long long M, unsigned long long *mismatches) {
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    unsigned int bad = 0;
    for (long long i = i0; i < M; i += stride) {
        const int c = (int)i;
        int r, col;
        win_index_split(w, c, r, col);
        bad += r != c / w.ncx || col != c % w.ncx;
    }
    if (bad) atomicAdd(mismatches, (unsigned long long)bad);
}
void launch_win_index_check(int ncx, int ncy, unsigned long long *mismatches, hipStream_t st) {
    const long long M = (long long)ncx * ncy;
    if (M > 0) hipLaunchKernelGGL(k_win_index_check, dim3((unsigned)std::min<long long>((M + 255) / 256, 8192)), dim3(256), 0, st, win_index_make(ncx, ncy), M, mismatches);
}

// ---- sum and sum of squares of the per-point distances as PCL forms them (a sequential loop adding floats to doubles,
// `sq_sum += d * d` with the product in float).  A parallel reduction gives the same bits whenever NO addition rounds:
// every value is a multiple of 2^q (q = the lowest set bit over all values) and the total is below 2^(q + 53), so every
// partial sum, in any order, is representable.  The kernel returns the sums and the two q's; the host checks the
// condition and falls back to the sequential loop otherwise: one far point (a near-zero disparity) or one cluster of near-duplicates
// is enough for that -- tests/cloud_range_fixtures.py's wide clouds, tests/test_gpu_cloud_filter_range.py.
__device__ __forceinline__ int low_bit_exp(float v) { // exponent of the lowest set bit of a finite float, INT_MAX for 0
    const unsigned int u = __float_as_uint(v) & 0x7fffffffu;
    if (u == 0u) return 0x7fffffff;
    const int e = (int)(u >> 23);
    const unsigned int m = u & 0x7fffffu;
    if (e == 0) return -149 + (__ffs((int)m) - 1);           // subnormal
    return (e - 150) + (m ? __ffs((int)m) - 1 : 23);
}
__global__ __launch_bounds__(256) void k_dist_stats(const float *__restrict__ dist, int64_t n, DistStats *__restrict__ out) {
    double s = 0.0, s2 = 0.0;
    int q1 = 0x7fffffff, q2 = 0x7fffffff, bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = dist[i];
        const float dd = __fmul_rn(d, d); // float * float, as in PCL
        bad |= !(d >= 0.0f) || !isfinite(dd);
        s += (double)d;
        s2 += (double)dd;
        q1 = min(q1, low_bit_exp(d));
        q2 = min(q2, low_bit_exp(dd));
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        s2 += __shfl_xor(s2, o);
        q1 = min(q1, __shfl_xor(q1, o));
        q2 = min(q2, __shfl_xor(q2, o));
        bad |= __shfl_xor(bad, o);
    }
    __shared__ double s_d[4][2];
    __shared__ int s_i[4][3];
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        s_d[w][0] = s, s_d[w][1] = s2;
        s_i[w][0] = q1, s_i[w][1] = q2, s_i[w][2] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) { // one set of atomics per workgroup; exact sums are order-free (see above)
        atomicAdd(&out->sum, (s_d[0][0] + s_d[1][0]) + (s_d[2][0] + s_d[3][0]));
        atomicAdd(&out->sq_sum, (s_d[0][1] + s_d[1][1]) + (s_d[2][1] + s_d[3][1]));
        atomicMin(&out->q_sum, min(min(s_i[0][0], s_i[1][0]), min(s_i[2][0], s_i[3][0])));
        atomicMin(&out->q_sq, min(min(s_i[0][1], s_i[1][1]), min(s_i[2][1], s_i[3][1])));
        if (s_i[0][2] | s_i[1][2] | s_i[2][2] | s_i[3][2]) atomicOr(&out->bad, 1);
    }
}

__global__ void k_keep_flags(const float *__restrict__ dist, int64_t n, double thr, unsigned int *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = !((double)dist[i] > thr); // removed: distances[i] > distance_threshold
}
__global__ void k_compact_kept(const float *__restrict__ xyz, const unsigned int *__restrict__ flag, const unsigned int *__restrict__ pos,
                               int64_t n, float *__restrict__ fxyz, int32_t *__restrict__ kept_index) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const unsigned int o = pos[i];
    fxyz[3 * (size_t)o] = xyz[3 * i];
    fxyz[3 * (size_t)o + 1] = xyz[3 * i + 1];
    fxyz[3 * (size_t)o + 2] = xyz[3 * i + 2];
    kept_index[o] = (int32_t)i;
}

__global__ void k_pack_filtered16(const double *__restrict__ xyz, const uint8_t *__restrict__ bgr, const int32_t *__restrict__ kept, int64_t m,
                                  uint4 *__restrict__ dst) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= m) return;
    const size_t i = (size_t)kept[o];
    uint4 v;
    v.x = __float_as_uint((float)xyz[3 * i]);
    v.y = __float_as_uint((float)xyz[3 * i + 1]);
    v.z = __float_as_uint((float)xyz[3 * i + 2]);
    v.w = (uint32_t)bgr[3 * i] | ((uint32_t)bgr[3 * i + 1] << 8) | ((uint32_t)bgr[3 * i + 2] << 16);
    dst[o] = v;
}
__global__ void k_f64_to_f32x3(const double *__restrict__ src, int64_t n3, float *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) dst[i] = (float)src[i]; // InsertPoint: pcl::PointXYZ(double, double, double) -> float (:61)
}

// (pixel-window pass) every finite point starts undecided; the others take no part in the searches (distance 0, as PCL)
__global__ void k_finite_flags(const float *__restrict__ xyz, int64_t n, unsigned int *__restrict__ flag, unsigned int *__restrict__ iota) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = (isfinite(xyz[3 * i]) && isfinite(xyz[3 * i + 1]) && isfinite(xyz[3 * i + 2])) ? 1u : 0u;
    iota[i] = (unsigned int)i;
}

__global__ void k_compact_list(const unsigned int *__restrict__ src, const unsigned int *__restrict__ flag, const unsigned int *__restrict__ pos,
                               int n, unsigned int *__restrict__ dst, int *__restrict__ count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) dst[pos[i]] = src[i];
    if (i == n - 1) *count = (int)(pos[i] + flag[i]);
}

// computePointNormal's covariance from the nine sums, the plane, flipNormalTowardsViewpoint(origin) + the turn toward CamCenter
__device__ float4 normal_from_sums(double a0, double a1, double a2, double a3, double a4, double a5, double a6, double a7, double a8, int cnt, const float4 p,
                                   float cx, float cy, float cz) {
    float4 out;
    if (cnt < 3) {
        out.x = out.y = out.z = out.w = __uint_as_float(0x7fc00000u);
    } else {
        const double inv = (double)cnt;
        a0 /= inv; a1 /= inv; a2 /= inv; a3 /= inv; a4 /= inv; a5 /= inv; a6 /= inv; a7 /= inv; a8 /= inv;
        double cov[9];
        cov[0] = a0 - a6 * a6;
        cov[1] = cov[3] = a1 - a6 * a7;
        cov[2] = cov[6] = a2 - a6 * a8;
        cov[4] = a3 - a7 * a7;
        cov[5] = cov[7] = a4 - a7 * a8;
        cov[8] = a5 - a8 * a8;
        double nv[3], curv;
        pcl_plane_from_cov(cov, nv, &curv);
        if ((0.0 - (double)p.x) * nv[0] + (0.0 - (double)p.y) * nv[1] + (0.0 - (double)p.z) * nv[2] < 0.0) {
            nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2];
        }
        float nx = (float)nv[0], ny = (float)nv[1], nz = (float)nv[2];
        const float vx = cx - p.x, vy = cy - p.y, vz = cz - p.z;
        if (nx * vx + ny * vy + nz * vz < 0.0f) { nx = -nx; ny = -ny; nz = -nz; } // :116-120
        out = make_float4(nx, ny, nz, (float)curv);
    }
    return out;
}

// normal_3d.h computePointNormal over the radius neighbourhood + flipNormalTowardsViewpoint(origin) + the turn toward
// CamCenter (CCloudOptimization.cpp:114-121); thread = sorted point, result stored at the point's original position
__global__ __launch_bounds__(256) void k_cloud_normals(const float4 *__restrict__ sxyz, const unsigned long long *__restrict__ keys, int n,
                                                        FGrid g, float r2, float cx, float cy, float cz, float4 *__restrict__ normals) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const float4 p = sxyz[j];
    int rs[9], re[9];
    ranges9(keys, n, g, p.x, p.y, p.z, rs, re);
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0;
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < 9; r++)
        for (int q = rs[r]; q < re[r]; q++) {
            const float4 o = sxyz[q];
            if (!(fdist2(p.x, p.y, p.z, o.x, o.y, o.z) < r2)) continue;
            const double x = o.x, y = o.y, z = o.z;
            a0 += x * x; a1 += x * y; a2 += x * z; a3 += y * y; a4 += y * z; a5 += z * z;
            a6 += x; a7 += y; a8 += z;
            cnt++;
        }
    normals[__float_as_uint(p.w)] = normal_from_sums(a0, a1, a2, a3, a4, a5, a6, a7, a8, cnt, p, cx, cy, cz);
}

// ---- normals on the pixel lattice (round 6).  The radius search of the normals is a window search too: every point within r of
// P lies inside the (2 w + 1)^2 pixels around P's own as soon as the window's bound (k_sor_window's: the distance from P to every
// ray at a pixel distance >= w + 1) exceeds r -- solved for w per point (win_bound.h: win_need); the lattice copy, with the removed points blanked, replaces
// the sort of the filtered cloud into a grid of r-cells and the walk over 27 of them.
__global__ __launch_bounds__(256) void k_normal_need(const float4 *__restrict__ lat, const unsigned int *__restrict__ cell_of, int64_t n, WinGeom g, double r,
                                                      int *__restrict__ wmax) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int need = 0;
    if (i < n) {
        const float4 P = lat[cell_of[i]];
        if (P.x == P.x) need = win_need(P, g, r);
    }
    need = wave_max(need);
    if ((threadIdx.x & 63) == 0 && need > *(volatile int *)wmax) atomicMax(wmax, need); // (same-address atomics retire ~88 per microsecond: one per wave was 0.7 ms)
}
__global__ void k_lattice_drop(const unsigned int *__restrict__ flag, const unsigned int *__restrict__ cell_of, int64_t n, float4 *__restrict__ lat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !flag[i]) lat[cell_of[i]].x = __uint_as_float(0x7fc00000u);
}
// thread = a point of the filtered cloud; the arithmetic of k_cloud_normals over the window's points (row by row instead of cell by cell)
__global__ __launch_bounds__(256) void k_normals_lattice(const float4 *__restrict__ lat, const unsigned int *__restrict__ cell_of,
                                                          const int32_t *__restrict__ kept_index, int64_t m, WinGeom g, double r, float r2, float cx, float cy,
                                                          float cz, float4 *__restrict__ normals) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4 p = make_float4(__uint_as_float(0x7fc00000u), 0.0f, 0.0f, 0.0f);
    unsigned int cell = 0;
    if (o < m) {
        cell = cell_of[kept_index[o]];
        p = lat[cell];
    }
    const bool live = p.x == p.x; // (a non-finite point has no lattice entry: its normal stays NaN)
    int w = live ? win_need(p, g, r) : 0;
    for (int t = 32; t > 0; t >>= 1) w = max(w, __shfl_xor(w, t)); // one window per wave: its points are neighbours on a row
    w = min(w, WIN_PAD);
    if (!live) return;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0, a8 = 0;
    int cnt = 0;
    for (int b = -w; b <= w; b++) {
        const float4 *row = lat + (size_t)cell + (ptrdiff_t)b * g.gw;
        for (int a = -w; a <= w; a++) {
            const float4 q = row[a];
            if (!(fdist2(p.x, p.y, p.z, q.x, q.y, q.z) < r2)) continue; // (NaN: a pixel without a point, or a removed one)
            const double x = q.x, y = q.y, z = q.z;
            a0 += x * x; a1 += x * y; a2 += x * z; a3 += y * y; a4 += y * z; a5 += z * z;
            a6 += x; a7 += y; a8 += z;
            cnt++;
        }
    }
    normals[o] = normal_from_sums(a0, a1, a2, a3, a4, a5, a6, a7, a8, cnt, p, cx, cy, cz);
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
// what the steps of one filter_cloud_device call share
struct FilterRun {
    FilterArena *A;
    hipStream_t st;
    const float *d_xyz;
    int64_t n, nv = 0; // points, finite points: only they take part in the searches (PCL: the k-d tree skips the others)
    int mean_k;
    const FilterLattice *pre;
    FilterRoute *route;
    float flo[3], fhi[3]; // the exact bounding box of the finite points (a sample's extremes are not the cloud's)
    int *d_cnt = nullptr;          // 4 ints
    DistStats *d_stats = nullptr;
    float *d_dist = nullptr;       // n each, from here on
    unsigned int *d_redo = nullptr, *d_redo2 = nullptr, *d_flag = nullptr, *d_pos = nullptr;
    const unsigned int *queries = nullptr; // the queries still undecided: d_redo, d_redo2, or the first grid level's point order
    int nq = 0;
    size_t mark = 0, mark_lat = 0; // the arena before the searches' buffers / behind the lattice copy
    WinGeom wg;                    // (with pre)
    float4 *lat = nullptr;         // the lattice copy and every point's place in it
    unsigned int *cell_of = nullptr;
    bool lat_kept = false;                    // no grid level has taken the lattice copy's arena space: the normals may use it
    bool prepassed = false, wave_done = false; // the tile pass ran / the wave passes ran
    float h_floor = 0.0f;                     // the ladder need not start below this search radius
    ScanTmp win_scan;                         // the tile pass's scan temporary, which the list and wave passes use again
    ScanTmp keep_scan;                        // the compaction's, which the radius outlier pass's compaction uses again
    int64_t nonfinite_kept = 0;               // non-finite points in the filtered cloud: they sort behind the finite ones in a grid over it
    FilterGridDev G;                          // the last grid level
    int64_t lat_cells() const { return prepassed ? (int64_t)wg.gw * (int64_t)wg.gh : 0; }
    void rewind() { A->off = lat_kept ? mark_lat : mark; }
};

// Of the `count` queries in R.queries, those whose flag is still up become the list (in order, in the buffer that is not being read)
// and R.nq their number: one host round trip.
int compact_undecided(FilterRun &R, int count, ScanTmp *keep = nullptr) {
    unsigned int *dst = (R.queries == R.d_redo) ? R.d_redo2 : R.d_redo;
    const int s = scan_u32(*R.A, R.d_flag, R.d_pos, (size_t)count, R.st, keep);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL(k_compact_list, blocks_for(count), dim3(256), 0, R.st, R.queries, R.d_flag, R.d_pos, count, dst, R.d_cnt);
    int *h_cnt = R.A->pin->cnt;
    DEVCHK(hipMemcpyAsync(h_cnt, R.d_cnt, sizeof(int), hipMemcpyDeviceToHost, R.st));
    DEVCHK(hipStreamSynchronize(R.st));
    R.queries = dst;
    R.nq = h_cnt[0];
    return RSM_OK;
}

// A pass through launch_sor_window_wave, for the caller's report (FilterLattice::passes_out): R.nq is already what it left over.
void report_wave_pass(FilterRun &R, int radius, int entered) {
    FilterPasses *P = R.pre->passes_out;
    if (!P || P->n >= FILTER_MAX_PASSES) return;
    P->radius[P->n] = radius;
    P->entered[P->n] = entered;
    P->decided[P->n] = entered - R.nq;
    P->workgroup[P->n] = entered <= R.pre->wg_max; // (launch_sor_window_wave's rule)
    P->n++;
}

// Step 2: the lattice copy (every finite point flagged undecided, d_redo2 = 0 .. n - 1) and the tile pass's window radius.
// Which window?  pre->radius > 0: the caller's; 0: the smallest of 7 / 12 / 16 pixels that decides >= 85 % of a sparse sample of the
// tiles (every 6th in x and y: ~3 % of the queries) -- a thin sheet (depth noise below the lateral spacing, the reference's rig
// geometry) is decided inside 15 x 15 pixels, a thick one (the synthetic bench rig: a disparity step of 0.05 pixel is 6 lateral
// spacings deep) needs 33 x 33; nothing decides enough: no window pass (*radius = 0).
int lattice_and_probe(FilterRun &R, int *radius_out) {
    const FilterLattice &L = *R.pre;
    R.lat = R.A->get<float4>(cloud_lattice_bytes(L.XL, L.XR, L.YL, L.YR) / sizeof(float4));
    R.cell_of = R.A->get<unsigned int>((size_t)R.n);
    if (!R.lat || !R.cell_of) return RSM_E_NOMEM;
    R.lat_kept = true;
    R.mark_lat = R.A->off;
    hipLaunchKernelGGL(k_finite_flags, blocks_for(R.n), dim3(256), 0, R.st, R.d_xyz, R.n, R.d_flag, R.d_redo2);
    launch_cloud_lattice(L, R.wg, R.n, R.lat, R.cell_of, R.st);
    int radius = L.radius;
    if (radius <= 0) {
        unsigned int *d_pc = (unsigned int *)R.d_cnt, *h_pc = (unsigned int *)R.A->pin->cnt; // (4 ints each)
        const int cand[3] = {7, 12, 16};
        for (int ci = 0; ci < 3 && radius <= 0; ci++) {
            DEVCHK(hipMemsetAsync(d_pc, 0, 3 * sizeof(unsigned int), R.st));
            launch_sor_window(R.lat, R.wg, R.mean_k, cand[ci], R.d_dist, R.d_flag, R.st, 6, d_pc);
            DEVCHK(hipMemcpyAsync(h_pc, d_pc, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, R.st));
            DEVCHK(hipStreamSynchronize(R.st));
            const double best = h_pc[0] ? (double)h_pc[1] / (double)h_pc[0] : 0.0;
            if (best >= 0.85 || (ci == 2 && best >= 0.5)) {
                radius = cand[ci];
                // every query this window leaves over has its (k+1)-th neighbour beyond the window's bound (closer points
                // cannot hide outside it): the ladder need not start below that scale
                float sum_lim;
                memcpy(&sum_lim, &h_pc[2], sizeof sum_lim);
                // (1.25 x the mean bound: a level at the bound itself would decide almost none of them)
                const float hf = 1.25f * sum_lim / (float)h_pc[0];
                if (std::isfinite(hf)) R.h_floor = hf;
            }
        }
    }
    if (L.radius_out) *L.radius_out = radius > 0 ? radius : 0;
    *radius_out = radius;
    return RSM_OK;
}

// Step 3: the tile pass over the whole lattice; what it cannot decide becomes the first query list.
int tile_pass(FilterRun &R, int radius) {
    launch_sor_window(R.lat, R.wg, R.mean_k, radius, R.d_dist, R.d_flag, R.st);
    R.queries = R.d_redo2;
    const int s = compact_undecided(R, (int)R.n, &R.win_scan);
    if (s != RSM_OK) return s;
    R.prepassed = true;
    if (R.pre->tile_left_out) *R.pre->tile_left_out = R.nq;
    return RSM_OK;
}

// Step 4: what a window below 24 pixels leaves over (a thick sheet's points whose neighbours spread wider: scattered, a seventh
// of C2's cloud) gets the 49 x 49 window a thread each, straight from the lattice copy (k_sor_window_list); what THAT
// leaves -- the points within a dozen pixels of the mask's border and of depth edges, whose neighbours lie on one
// side: 1.6 % of C2's cloud, the queries that cost the grid ladder most (coarse levels: tens of thousands of
// candidates in the 27 cells of each) -- an 81 x 81 window; only the rest (holes, outliers, islands) goes on.
// *last: in, the tile pass's radius; out, the widest window run.
int list_passes(FilterRun &R, int *last) {
    const FilterLattice &L = *R.pre;
    const int radii[2] = {24, 40};
    for (int pass = 0; pass < 2 && R.nq > 0; pass++) {
        if (radii[pass] <= *last || !((L.list_pass >> pass) & 1)) continue;
        const bool wave = (L.list_pass >> (3 + pass)) & 1; // (A/B: the wave form at this radius instead of the thread form)
        const int entered = R.nq;
        if (wave) launch_sor_window_wave(R.lat, R.cell_of, R.wg, R.mean_k, radii[pass], R.queries, R.nq, R.d_dist, R.d_flag, R.st, L.wg_max);
        else launch_sor_window_list(R.lat, R.cell_of, R.wg, R.mean_k, radii[pass], R.queries, R.nq, R.d_dist, R.d_flag, R.st);
        const int s = compact_undecided(R, R.nq, &R.win_scan);
        if (s != RSM_OK) return s;
        if (wave) report_wave_pass(R, radii[pass], entered);
        *last = radii[pass]; // (the ladder keeps its start: what is left now is few, and a level whose 27 cells hold tens of
                             // thousands of candidates costs a wave-per-query search milliseconds however few the queries)
    }
    return RSM_OK;
}

// Step 5: what the list passes leave (C2: 564 of 5.5 M -- mask corners, hole rims, outliers): a wave each over windows of 80, 160,
// 320 ... pixels of the lattice copy, while there are few enough for that to be cheaper than a grid level (a level is a
// sort of the whole cloud plus, for these queries, 27 cells of tens of thousands of candidates each: 4 ms a level on C2).
int wave_passes(FilterRun &R, int last) {
    const FilterLattice &L = *R.pre;
    const int span = std::max(L.XR - L.XL, L.YR - L.YL) + 1;
    for (int wr = std::max(80, 2 * last); R.nq > 0 && R.nq <= 65536; wr *= 2) {
        const int entered = R.nq;
        launch_sor_window_wave(R.lat, R.cell_of, R.wg, R.mean_k, wr, R.queries, R.nq, R.d_dist, R.d_flag, R.st, L.wg_max);
        const int s = compact_undecided(R, R.nq, &R.win_scan);
        if (s != RSM_OK) return s;
        report_wave_pass(R, wr, entered);
        if (wr >= span) break; // the window already covers the whole box: what is left has fewer than k + 1 points within its bound
    }
    R.wave_done = true;
    return RSM_OK;
}

// Step 6, the grid ladder.
// first cell edge: ~sqrt(k + 1) point spacings of a surface patch whose area is the product of the two largest
// robust extents; queries that cannot be decided inside their 27 cells (fewer than k + 1 points within h: thick or
// sparse parts of the cloud, patch corners, isolated points) are retried on a grid with twice the edge; what is left
// after KNN_LEVELS grids (or once only a handful remain) is searched against all points by the whole chip.
// One cell edge does not fit a whole cloud: a perspective depth map is 25 times denser (per unit of space) in its near
// part than in its far part (C2: 1.25 vs 6 units between neighbours), and the surface estimate above is off for a deep
// or thick one.  The search therefore runs over a ladder of grids from fine to coarse, h doubling: a query is decided
// at the first level whose 27 cells hold its k + 1 nearest (there its candidates number a few hundred whatever the
// local density); an undecided attempt costs one table lookup and one count over the few candidates a too-fine grid
// offers.  Every level re-sorts the points (0.65 ms for 5.5 M): cheap next to one query pass with a wrong h
// (a single level at the surface estimate ran the near part's queries over ~50 000 candidates each: 390 ms).
// The ladder starts one octave below the surface estimate (on C2 two octaves below decides 10 % of the queries for
// a quarter of the search time, three octaves below nothing).
// All of it only when a grid is built at all: the cloud of a matched pair is searched on its pixel lattice and the sample, its
// round trip and its quantiles stay out of the call.
int grid_ladder(FilterRun &R) {
    const int KNN_LEVELS = 12;
    float lo[3], hi[3], glo[3], ghi[3];
    if (!sample_extent(R.A, R.d_xyz, R.n, R.st, lo, hi)) return RSM_E_HIP;
    double e[3] = {(double)hi[0] - lo[0], (double)hi[1] - lo[1], (double)hi[2] - lo[2]};
    std::sort(e, e + 3);
    const double area = std::max(e[2] * e[1], 1e-12), spacing = sqrt(area / (0.98 * 0.98 * 0.98 * (double)std::max<int64_t>(R.nv, 1)));
    float h = (float)(spacing * sqrt((double)(R.mean_k + 1)));
    if (!(h > 0.0f) || !std::isfinite(h)) h = 1.0f;
    // the grid box: the robust extent grown by a few cells, inside the exact bounding box (far outliers are clamped
    // into the border cells instead of blowing up the cell count)
    for (int a = 0; a < 3; a++) {
        glo[a] = std::max(R.flo[a], lo[a] - 4.0f * h);
        ghi[a] = std::min(R.fhi[a], hi[a] + 4.0f * h);
        if (!(ghi[a] >= glo[a])) ghi[a] = glo[a];
    }
    h *= 0.5f;
    if (R.h_floor > h) h = R.h_floor;
    if (R.route && R.route->h0 > 0.0f) h = R.route->h0; // (a level decides a query only with all of its k + 1 nearest in hand: any start gives the same bits)
    for (int level = 0; level < KNN_LEVELS && R.nq > 0; level++, h *= 2.0f) {
        R.A->off = R.mark; // the previous level's grid is done (its kernels are ordered before this level's on the stream)
        R.lat_kept = false; // (the grid takes the lattice copy's arena space: R.lat and R.cell_of dangle from here on, only lat_kept says so)
        FilterGridDev &G = R.G;
        int s = build_grid(R.A, R.d_xyz, R.n, R.nv, h, glo, ghi, R.st, G);
        if (s != RSM_OK) return s;
        if (R.route) {
            FilterRoute *route = R.route;
            if (level == 0) {
                route->h = h;
                route->kind0 = G.table_kind;
                const int nk[3] = {G.g.nx, G.g.ny, G.g.nz}, pk[3] = {G.g.p0, G.g.p1, G.g.p2};
                for (int a = 0; a < 3; a++) {
                    route->origin[a] = glo[a];
                    route->cells[pk[a]] = nk[a];
                }
            }
            route->levels++;
            route->kinds |= 1 << G.table_kind;
        }
        if (level == 0 && !R.prepassed) R.queries = G.vals; // every point, in grid order (coherent waves)
        launch_knn(R.d_xyz, G, (int)R.nv, h, R.mean_k, R.queries, R.nq, R.d_dist, R.d_flag, R.st);
        if ((s = compact_undecided(R, R.nq)) != RSM_OK) return s; // undecided queries -> the next level's list, in order
        if (R.nq <= 48) break; // cheaper to finish against all points than to sort again (a coarser level costs ~0.8 ms, the
                               // whole-chip search ~25 us per query)
    }
    return RSM_OK;
}

// Step 7: the queries still left against ALL points (k_xq_*), read from any array that holds every finite point once: the last grid
// level's sorted copy, still in the arena, or -- no level ran -- the lattice copy (its empty pixels are NaN: never below any threshold)
int whole_chip_search(FilterRun &R, bool over_lattice) {
    XqState *d_xq = R.A->get<XqState>((size_t)XQ_BATCH);
    int *d_hist = R.A->get<int>((size_t)XQ_BATCH * 2048);
    if (!d_xq || !d_hist) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(d_hist, 0, sizeof(int) * (size_t)XQ_BATCH * 2048, R.st));
    const float4 *arr = over_lattice ? R.lat : R.G.sxyz;
    const int arr_n = over_lattice ? (int)R.lat_cells() : (int)R.nv;
    if (!arr || R.lat_cells() >= (1ll << 31)) return RSM_E_INVALID;
    for (int q0 = 0; q0 < R.nq; q0 += XQ_BATCH) {
        const int cnt = std::min(XQ_BATCH, R.nq - q0);
        launch_xq_search(R.d_xyz, arr, arr_n, R.queries + q0, cnt, d_xq, d_hist, R.mean_k, (int)R.nv, R.d_dist, R.st);
    }
    return RSM_OK;
}

// Step 8: mean / stddev exactly as PCL forms them (a sequential loop over the per-point distances in point order): on the
// device when no addition can round (k_dist_stats), else on the host; *thr = the removal threshold.  need_r > 0: the widest window a
// normal's radius search of that radius needs on the lattice comes back with the statistics (pin->cnt[3]; 1 << 20 when not asked).
int distance_threshold(FilterRun &R, double std_mul, double need_r, double stats[4], double *thr) {
    DistStats *h_stats = &R.A->pin->stats;
    int *h_cnt = R.A->pin->cnt;
    double sum = 0.0, sq_sum = 0.0;
    const DistStats init{0.0, 0.0, 0x7fffffff, 0x7fffffff, 0};
    *h_stats = init;
    DEVCHK(hipMemcpyAsync(R.d_stats, h_stats, sizeof init, hipMemcpyHostToDevice, R.st));
    hipLaunchKernelGGL(k_dist_stats, dim3((unsigned)std::min<int64_t>((R.n + 255) / 256, 1024)), dim3(256), 0, R.st, R.d_dist, R.n, R.d_stats);
    h_cnt[3] = 1 << 20;
    if (need_r > 0.0) {
        DEVCHK(hipMemsetAsync(R.d_cnt + 3, 0, sizeof(int), R.st));
        hipLaunchKernelGGL(k_normal_need, blocks_for(R.n), dim3(256), 0, R.st, R.lat, R.cell_of, R.n, R.wg, need_r, R.d_cnt + 3);
        DEVCHK(hipMemcpyAsync(h_cnt + 3, R.d_cnt + 3, sizeof(int), hipMemcpyDeviceToHost, R.st));
    }
    DEVCHK(hipMemcpyAsync(h_stats, R.d_stats, sizeof init, hipMemcpyDeviceToHost, R.st));
    DEVCHK(hipStreamSynchronize(R.st));
    auto exact = [](double total, int q) { // every partial sum is a multiple of 2^q below 2^(q + 53)
        if (q == 0x7fffffff) return true;   // all zero
        return total * (1.0 + 1e-9) < ldexp(1.0, q + 53);
    };
    if (!h_stats->bad && exact(h_stats->sum, h_stats->q_sum) && exact(h_stats->sq_sum, h_stats->q_sq)) {
        sum = h_stats->sum;
        sq_sum = h_stats->sq_sum;
    } else {
        std::vector<float> hd((size_t)R.n);
        DEVCHK(hipMemcpyAsync(hd.data(), R.d_dist, sizeof(float) * (size_t)R.n, hipMemcpyDeviceToHost, R.st));
        DEVCHK(hipStreamSynchronize(R.st));
        for (int64_t i = 0; i < R.n; i++) {
            sum += hd[(size_t)i];
            sq_sum += hd[(size_t)i] * hd[(size_t)i]; // float * float, as in PCL
        }
    }
    const double mean = sum / (double)R.nv; // valid_distances
    const double variance = (sq_sum - sum * sum / (double)R.nv) / ((double)R.nv - 1);
    const double stddev = sqrt(variance);
    *thr = mean + std_mul * stddev;
    if (stats) {
        stats[0] = mean;
        stats[1] = stddev;
        stats[2] = *thr;
        stats[3] = (double)R.nq; // what the whole-chip search took
    }
    return RSM_OK;
}

// Step 9: d_flag = kept, the kept points and their indices in order, *m = their number (one host round trip)
int compact_kept(FilterRun &R, float *d_fxyz, int32_t *d_kept_index, int64_t *m) {
    int s = scan_u32(*R.A, R.d_flag, R.d_pos, (size_t)R.n, R.st, &R.keep_scan);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL(k_compact_kept, blocks_for(R.n), dim3(256), 0, R.st, R.d_xyz, R.d_flag, R.d_pos, R.n, d_fxyz, d_kept_index);
    uint64_t total = 0;
    if ((s = scan_total(R.d_flag, R.d_pos, (size_t)R.n, R.st, &total, (unsigned int *)R.A->pin->cnt)) != RSM_OK) return s;
    *m = (int64_t)total;
    return RSM_OK;
}
int keep_compact(FilterRun &R, double thr, float *d_fxyz, int32_t *d_kept_index, int64_t *m) {
    hipLaunchKernelGGL(k_keep_flags, blocks_for(R.n), dim3(256), 0, R.st, R.d_dist, R.n, thr, R.d_flag);
    return compact_kept(R, d_fxyz, d_kept_index, m);
}

// the radius outlier pass's count on the grid route: the n points of d_xyz (nv of them finite, inside [lo, hi]) sorted into a grid with cell
// edge = the search radius, d_count[i] = min(count(p_i), cap); the non-finite points sort behind the finite ones and keep count 0
int radius_count_on_grid(FilterArena *A, const float *d_xyz, int64_t n, int64_t nv, const float lo[3], const float hi[3], double radius, int cap,
                         int32_t *d_count, hipStream_t st) {
    DEVCHK(hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)n, st));
    if (nv <= 0) return RSM_OK;
    FilterGridDev G;
    const int s = build_grid(A, d_xyz, n, 0 /* no table: the count walks its ranges by binary search, as the normals do */, (float)radius, lo, hi, st, G);
    if (s != RSM_OK) return s;
    launch_radius_count_grid(G, (int)nv, (float)(radius * radius), cap, d_count, st);
    return RSM_OK;
}

// Step 9b, the radius outlier pass (k_filter_outrem.hip) on the m points step 9 kept: their counts -- on the lattice copy, with the points
// step 9 removed blanked, or on a grid of radius-cells over d_fxyz --, d_flag = survives both passes, and step 9's compaction again.
// The counts take d_redo (the searches' query lists are done), so the pass adds no buffer to the arena.
int outrem_pass(FilterRun &R, FilterOutrem &O, double thr, int lattice_window, float *d_fxyz, int32_t *d_kept_index, int64_t *m) {
    const int64_t m0 = *m;
    const int64_t nonfinite = (0.0 > thr) ? 0 : R.n - R.nv; // step 9 keeps a non-finite point (distance 0) unless the threshold is negative
    const int cap = O.min_neighbors < 0x7fffffff ? O.min_neighbors + 1 : 0x7fffffff;
    int32_t *d_count = (int32_t *)R.d_redo;
    if (lattice_window > 0) {
        DEVCHK(hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)m0, R.st));
        hipLaunchKernelGGL(k_lattice_drop, blocks_for(R.n), dim3(256), 0, R.st, R.d_flag, R.cell_of, R.n, R.lat);
        launch_radius_count_lattice(R.lat, R.cell_of, d_kept_index, m0, R.wg, O.radius, (float)(O.radius * O.radius), cap, d_count, R.st);
    } else {
        R.A->off = R.mark; // (the grid takes the lattice copy's arena space, and the compaction's scan temporary's)
        R.lat_kept = false;
        R.keep_scan = ScanTmp{};
        const int s = radius_count_on_grid(R.A, d_fxyz, m0, m0 - nonfinite, R.flo, R.fhi, O.radius, cap, d_count, R.st);
        if (s != RSM_OK) return s;
        R.A->off = R.mark;
    }
    launch_outrem_flags(d_count, R.d_pos, R.n, O.min_neighbors, R.d_flag, R.st);
    const int s = compact_kept(R, d_fxyz, d_kept_index, m);
    if (s != RSM_OK) return s;
    R.nonfinite_kept = 0; // (count 0: every one of them went)
    O.points_in = m0;
    O.removed = m0 - *m;
    O.nonfinite = nonfinite;
    O.window = lattice_window;
    return RSM_OK;
}

// Step 10, on the lattice copy with the removed points blanked: a window of w pixels holds every normal's neighbourhood
int normals_on_lattice(FilterRun &R, int64_t m, const int32_t *d_kept_index, double normal_radius, const float cam_center[3], float4 *d_normals) {
    hipLaunchKernelGGL(k_lattice_drop, blocks_for(R.n), dim3(256), 0, R.st, R.d_flag, R.cell_of, R.n, R.lat);
    DEVCHK(hipMemsetD32Async((hipDeviceptr_t)d_normals, 0x7fc00000, (size_t)4 * m, R.st));
    hipLaunchKernelGGL(k_normals_lattice, blocks_for(m), dim3(256), 0, R.st, R.lat, R.cell_of, d_kept_index, m, R.wg, normal_radius,
                       (float)(normal_radius * normal_radius), cam_center[0], cam_center[1], cam_center[2], d_normals);
    DEVCHK(hipStreamSynchronize(R.st));
    DEVCHK(hipGetLastError());
    return RSM_OK;
}
// ... or on a grid with cell edge = search radius; the non-finite points (all kept: distance 0) sort behind the finite ones and keep
// the NaN normal the buffer is filled with
int normals_on_grid(FilterRun &R, int64_t m, const float *d_fxyz, double normal_radius, const float cam_center[3], float4 *d_normals) {
    FilterGridDev G2;
    const int64_t mv = m - R.nonfinite_kept;
    const int s = build_grid(R.A, d_fxyz, m, 0 /* no table: the normals walk their ranges by binary search */, (float)normal_radius, R.flo, R.fhi, R.st, G2);
    if (s != RSM_OK) return s;
    const float r2 = (float)(normal_radius * normal_radius);
    DEVCHK(hipMemsetD32Async((hipDeviceptr_t)d_normals, 0x7fc00000, (size_t)4 * m, R.st));
    if (mv > 0)
        hipLaunchKernelGGL(k_cloud_normals, blocks_for(mv), dim3(256), 0, R.st, G2.sxyz, G2.keys, (int)mv, G2.g, r2, cam_center[0], cam_center[1], cam_center[2],
                           d_normals);
    DEVCHK(hipStreamSynchronize(R.st));
    DEVCHK(hipGetLastError());
    return RSM_OK;
}
} // namespace

// d_xyz: n x 3 float (device).  Outputs (device): kept_index [n] (first *n_kept valid), fxyz [3n], normals [n] float4.
// A: reserved by the caller (filter_arena_reserve) with at least filter_arena_bytes(n) free.
// pre (optional): the cloud is the depth map of a matched pair -- its pixel lattice decides most queries (k_sor_window),
// the grid ladder only sees the rest.
int filter_cloud_device(FilterArena *A, const float *d_xyz, int64_t n, int mean_k, double std_mul, double normal_radius,
                        const float cam_center[3], int32_t *d_kept_index, float *d_fxyz, float4 *d_normals, int64_t *n_kept,
                        double stats[4], hipStream_t st, const FilterLattice *pre, FilterRoute *route) {
    *n_kept = 0;
    if (route) {
        const FilterRoute in = *route;
        *route = FilterRoute{};
        route->h0 = in.h0;
        route->outrem.on = in.outrem.on, route->outrem.min_neighbors = in.outrem.min_neighbors, route->outrem.radius = in.outrem.radius;
        if (in.outrem.on) route->outrem.points_in = 0;
    }
    FilterOutrem *const outrem = route && route->outrem.on ? &route->outrem : nullptr;
    if (pre && pre->passes_out) *pre->passes_out = FilterPasses{};
    if (n <= 0) return RSM_OK;
    if (n >= (1ll << 31) || mean_k < 1 || !A) return RSM_E_INVALID;
    FilterRun R;
    R.A = A, R.st = st, R.d_xyz = d_xyz, R.n = n, R.mean_k = mean_k, R.pre = pre, R.route = route;
    int s = cloud_bbox(A, d_xyz, n, st, R.flo, R.fhi, &R.nv); // step 1
    if (s != RSM_OK) return s;
    R.d_cnt = A->get<int>(4);
    R.d_stats = A->get<DistStats>(1);
    R.d_dist = A->get<float>((size_t)n);
    R.d_redo = A->get<unsigned int>((size_t)n), R.d_redo2 = A->get<unsigned int>((size_t)n);
    R.d_flag = A->get<unsigned int>((size_t)n), R.d_pos = A->get<unsigned int>((size_t)n);
    if (A->failed) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(R.d_dist, 0, sizeof(float) * (size_t)n, st)); // non-finite points: distance 0, as PCL
    R.nq = (int)R.nv;
    R.nonfinite_kept = n - R.nv; // (all kept: distance 0)
    R.mark = R.mark_lat = A->off;
    if (pre && mean_k <= 128 && R.nv > 0) { // the pixel-window passes: what they cannot decide becomes the ladder's first query list
        R.wg = win_geom(*pre);
        int radius = 0;
        if ((s = lattice_and_probe(R, &radius)) != RSM_OK) return s;
        if (radius > 0) {
            if ((s = tile_pass(R, radius)) != RSM_OK || (s = list_passes(R, &radius)) != RSM_OK) return s;
            if ((pre->list_pass & 4) && radius >= 24 && (s = wave_passes(R, radius)) != RSM_OK) return s;
            if (pre->undecided_out) *pre->undecided_out = R.nq;
        }
    }
    // after the wave passes a handful is left at most (isolated points): straight to the whole-chip search, over the lattice copy
    // as the point array -- no grid level, no sort
    const bool skip_ladder = R.wave_done && R.nq <= 48;
    FilterPasses *const report = pre ? pre->passes_out : nullptr;
    if (report && !skip_ladder) report->ladder_in = R.nq;
    if (R.nq > 0 && !skip_ladder && (s = grid_ladder(R)) != RSM_OK) return s;
    if (report) report->whole_in = R.nq, report->whole_over_lattice = R.nq > 0 && skip_ladder;
    if (R.nq > 0 && (s = whole_chip_search(R, skip_ladder)) != RSM_OK) return s;
    R.rewind();
    double thr = 0.0;
    // (the normals' window is asked for while the lattice copy is still there and the caller lets them use it)
    // (... and the radius outlier pass's: a window that covers the larger of the two radii covers the smaller)
    const bool ask = R.lat_kept && (d_normals || outrem) && pre->normals_wmax > 0;
    const double need_r = std::max(d_normals ? normal_radius : 0.0, outrem ? outrem->radius : 0.0);
    if ((s = distance_threshold(R, std_mul, ask ? need_r : 0.0, stats, &thr)) != RSM_OK) return s;
    int64_t m = 0;
    if ((s = keep_compact(R, thr, d_fxyz, d_kept_index, &m)) != RSM_OK) return s;
    if (outrem && m > 0) { // on the lattice copy under the normals' rule below, else on a grid
        const int need = A->pin->cnt[3];
        const bool on_lattice = R.lat_kept && need <= pre->normals_wmax;
        if ((s = outrem_pass(R, *outrem, thr, on_lattice ? std::max(need, 1) : 0, d_fxyz, d_kept_index, &m)) != RSM_OK) return s;
    }
    *n_kept = m;
    if (m > 0 && d_normals) {
        // normals of the filtered cloud.  On the lattice copy when it is still there and a window of at most pre->normals_wmax pixels holds every
        // normal's neighbourhood (k_normal_need: a property of the rig -- the search radius in pixel spacings at the nearest point)
        const int need = A->pin->cnt[3];
        if (pre && pre->normals_out) {
            pre->normals_out[0] = 0;
            pre->normals_out[1] = R.lat_kept ? need : -1;
        }
        if (R.lat_kept && need <= pre->normals_wmax) {
            if (pre->normals_out) pre->normals_out[0] = std::max(need, 1);
            s = normals_on_lattice(R, m, d_kept_index, normal_radius, cam_center, d_normals);
        } else {
            A->off = R.mark;
            s = normals_on_grid(R, m, d_fxyz, normal_radius, cam_center, d_normals);
        }
        if (s != RSM_OK) return s;
    }
    A->off = R.mark;
    return RSM_OK;
}

int radius_count_device(FilterArena *A, const float *d_xyz, int64_t n, double radius, int cap, int32_t *d_count, hipStream_t st) {
    if (n <= 0) return RSM_OK;
    if (n >= (1ll << 31) || cap < 1 || !A) return RSM_E_INVALID;
    const size_t mark = A->off;
    float lo[3], hi[3];
    int64_t nv = 0;
    int s = cloud_bbox(A, d_xyz, n, st, lo, hi, &nv);
    if (s == RSM_OK) s = radius_count_on_grid(A, d_xyz, n, nv, lo, hi, radius, cap, d_count, st);
    if (s != RSM_OK) return s;
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    A->off = mark;
    return RSM_OK;
}

void launch_f64_to_f32x3(const double *src, int64_t n, float *dst, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_f64_to_f32x3, dim3((unsigned)((3 * n + 255) / 256)), dim3(256), 0, st, src, 3 * n, dst);
}
void launch_pack_filtered16(const double *xyz, const uint8_t *bgr, const int32_t *kept, int64_t m, void *dst, hipStream_t st) {
    if (m > 0) hipLaunchKernelGGL(k_pack_filtered16, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, xyz, bgr, kept, m, (uint4 *)dst);
}
