// cloud_grid.h -- the radius-cell grid of the cloud kernels (k_filter_knn.hip's searches, k_filter.hip's normals, k_mls.hip; built by cloud_grid.hip) and PCL's eigen33
// in double.
// Points sorted by the key of a uniform grid (cell edge h): the 27 cells around a point are 9 contiguous ranges of the
// sorted array (ranges9), found by binary search on the keys.
#pragma once

#include "cloud_arena.h"
#include "dev_prims.h"

// Grid in KEY order: axis "x" is the fastest digit of the cell key, and it is the WORLD axis with the most cells (p0) --
// a depth map is a sheet in a deep box, so the rows of cells along its depth hold a handful of points each and the
// per-row table + short search inside the row (table kind 2) stays cheap when the cells are too many for a table.
struct FGrid {
    double ox, oy, oz, inv_h; // origin (the box's low corner, floats), 1 / the cell edge H = grid_edge(h)
    int nx, ny, nz;
    int p0, p1, p2; // world axis (0 = x, 1 = y, 2 = z) of key axis x, y, z
};
__device__ __forceinline__ float pick_axis(int a, float x, float y, float z) { return a == 0 ? x : (a == 1 ? y : z); }

__device__ __forceinline__ float fdist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// The searches rest on one invariant: every point q that passes a membership test against p -- fdist2(p, q) <= fl(h h) for the
// k nearest, fdist2(p, q) < fl32(r r) with h = fl32(r) for the radius searches -- lies at most one cell from p on each axis.
// The bound (u = 2^-24, float32; e = 2^-53, double):
//   fdist2 is a rounded sum of the non-negative fl(d_a^2), so fl(d_a^2) <= T on each axis, d_a = fl(p_a - q_a): |d_a| <= sqrt(T) (1 + u/2)
//   and |p_a - q_a| <= |d_a| (1 + u); sqrt(T) <= h (1 + 3u/2) for both tests.  So |p_a - q_a| <= h (1 + 3u) < h (1 + 2^-22)
//   (for h^2 a normal float; below 2^-63 the accepted differences are below 2^-63: the edge's floor).
//   cell_of evaluates t = fl64(fl64(v - o) s), s = fl64(1 / H), in double: |t - (v - o) / H| <= 3e |t|, and a pair that clamping
//   could not merge has |t| <= n + 2 <= 2^20 + 2 on both ends: t_p - t_q <= (h / H)(1 + 2^-22)(1 + e) + 2^-30.
//   With H = grid_edge(h) = h (1 + 2^-20) that is < 1, so floor(t_p) - floor(t_q) <= 1; clamping to [0, n - 1] keeps it.
// (The float form, floorf(fl32(v - o) * fl32(1 / h)), has no such bound: its rounding of v - o alone puts pairs at a float distance
// below r into cells two apart -- tests/cloud_probes.py builds them, tests/test_gpu_cloud_grid_edges.py runs them.)
__host__ __device__ __forceinline__ double grid_edge(float h) {
    const double H = (double)h * (1.0 + 0x1p-20);
    return H > 0x1p-62 ? H : 0x1p-62;
}
__device__ __forceinline__ int cell_of(float v, double o, double inv_h, int n) {
    const double t = floor(((double)v - o) * inv_h);
    return (int)fmin(fmax(t, 0.0), (double)(n - 1)); // (clamped in double: no out-of-range conversion for far points)
}
// cell of a world point, in key order
__device__ __forceinline__ void grid_cell(const FGrid &g, float x, float y, float z, int &ix, int &iy, int &iz) {
    ix = cell_of(pick_axis(g.p0, x, y, z), g.ox, g.inv_h, g.nx);
    iy = cell_of(pick_axis(g.p1, x, y, z), g.oy, g.inv_h, g.ny);
    iz = cell_of(pick_axis(g.p2, x, y, z), g.oz, g.inv_h, g.nz);
}

__device__ __forceinline__ int lower_bound_key(const unsigned long long *__restrict__ keys, int n, unsigned long long k) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the 9 contiguous ranges of the sorted array that hold the 27 cells around p (binary search on the keys; used by the
// normals and by the k-nearest search when the grid has too many cells for a table)
// range t of 9 around the cell (ix, iy, iz): the up to 3 x-adjacent cells of the row of cells (iy + t % 3 - 1, iz + t / 3 - 1)
__device__ __forceinline__ void range_of9(const unsigned long long *__restrict__ keys, int n, const FGrid &g, int ix, int iy, int iz, int t, int &rs, int &re) {
    const int x0 = max(ix - 1, 0), x1 = min(ix + 1, g.nx - 1);
    const int yy = iy + t % 3 - 1, zz = iz + t / 3 - 1;
    if (yy < 0 || yy >= g.ny || zz < 0 || zz >= g.nz) {
        rs = re = 0;
        return;
    }
    const unsigned long long base = ((unsigned long long)zz * g.ny + yy) * g.nx;
    rs = lower_bound_key(keys, n, base + x0);
    re = lower_bound_key(keys, n, base + x1 + 1);
}
__device__ __forceinline__ void ranges9(const unsigned long long *__restrict__ keys, int n, const FGrid &g, float px, float py,
                                        float pz, int (&rs)[9], int (&re)[9]) {
    int ix, iy, iz;
    grid_cell(g, px, py, pz, ix, iy, iz);
#pragma unroll
    for (int t = 0; t < 9; t++) range_of9(keys, n, g, ix, iy, iz, t, rs[t], re[t]);
}

// ---- eigen33 / computeRoots of PCL's common/impl/eigen.hpp (smallest eigenvalue and its vector), in double
__device__ __forceinline__ void pcl_roots2(double b, double c, double *r) {
    r[0] = 0.0;
    double d = b * b - 4.0 * c;
    if (d < 0.0) d = 0.0;
    const double sd = sqrt(d);
    r[2] = 0.5 * (b + sd);
    r[1] = 0.5 * (b - sd);
}
__device__ inline void pcl_plane_from_cov(const double *cov, double *nrm, double *curvature) {
    double scale = 0.0;
    for (int i = 0; i < 9; i++) scale = fmax(scale, fabs(cov[i]));
    if (scale <= 2.2250738585072014e-308) scale = 1.0;
    double m[9];
    for (int i = 0; i < 9; i++) m[i] = cov[i] / scale;
    double r[3];
    const double c0 = m[0] * m[4] * m[8] + 2.0 * m[1] * m[2] * m[5] - m[0] * m[5] * m[5] - m[4] * m[2] * m[2] - m[8] * m[1] * m[1];
    const double c1 = m[0] * m[4] - m[1] * m[1] + m[0] * m[8] - m[2] * m[2] + m[4] * m[8] - m[5] * m[5];
    const double c2 = m[0] + m[4] + m[8];
    if (fabs(c0) < 2.220446049250313e-16) {
        pcl_roots2(c2, c1, r);
    } else {
        const double s_inv3 = 1.0 / 3.0, s_sqrt3 = sqrt(3.0);
        const double c2_over_3 = c2 * s_inv3;
        double a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
        if (a_over_3 > 0.0) a_over_3 = 0.0;
        const double half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1));
        double q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
        if (q > 0.0) q = 0.0;
        const double rho = sqrt(-a_over_3);
        const double theta = atan2(sqrt(-q), half_b) * s_inv3;
        const double ct = cos(theta), st = sin(theta);
        r[0] = c2_over_3 + 2.0 * rho * ct;
        r[1] = c2_over_3 - rho * (ct + s_sqrt3 * st);
        r[2] = c2_over_3 - rho * (ct - s_sqrt3 * st);
        if (r[0] >= r[1]) { const double t = r[0]; r[0] = r[1]; r[1] = t; }
        if (r[1] >= r[2]) {
            const double t = r[1]; r[1] = r[2]; r[2] = t;
            if (r[0] >= r[1]) { const double u = r[0]; r[0] = r[1]; r[1] = u; }
        }
        if (r[0] <= 0.0) pcl_roots2(c2, c1, r);
    }
    const double ev = r[0] * scale;
    m[0] -= r[0];
    m[4] -= r[0];
    m[8] -= r[0];
    const double v1[3] = {m[1] * m[5] - m[2] * m[4], m[2] * m[3] - m[0] * m[5], m[0] * m[4] - m[1] * m[3]};
    const double v2[3] = {m[1] * m[8] - m[2] * m[7], m[2] * m[6] - m[0] * m[8], m[0] * m[7] - m[1] * m[6]};
    const double v3[3] = {m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]};
    const double l1 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2];
    const double l2 = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
    const double l3 = v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2];
    const double *v = v3;
    double l = l3;
    if (l1 >= l2 && l1 >= l3) { v = v1; l = l1; }
    else if (l2 >= l1 && l2 >= l3) { v = v2; l = l2; }
    const double s = sqrt(l);
    for (int i = 0; i < 3; i++) nrm[i] = v[i] / s;
    const double tr = cov[0] + cov[4] + cov[8];
    *curvature = (tr != 0.0) ? fabs(ev / tr) : 0.0;
}

struct FilterGridDev {
    unsigned long long *keys = nullptr;
    unsigned int *vals = nullptr; // original index of every sorted point
    float4 *sxyz = nullptr;
    int2 *table = nullptr; // (first, one past last) sorted index per cell (table_kind 1) or per (y, z) row of cells (2)
    int table_kind = 0;    // 0: none, binary search on all keys
    FGrid g{};
};

// cloud_grid.hip: sorts the n points of d_xyz (n x 3 float) by the key of a grid for the search radius h -- cell edge grid_edge(h) --
// over the box [bb_lo, bb_hi] (points outside fall into the border cells: clamping is non-expansive, so two points within h of each
// other still sit in adjacent cells; non-finite points sort behind every cell); nv = finite points, 0 = no cell table (ranges by
// binary search).  The arrays come from the arena and stay allocated until its caller rewinds it.
int build_grid(FilterArena *A, const float *d_xyz, int64_t n, int64_t nv, float h, const float bb_lo[3], const float bb_hi[3],
               hipStream_t st, FilterGridDev &G);
// the exact bounding box of the finite points of d_xyz and their number (one host round trip; its 8 device words stay allocated)
int cloud_bbox(FilterArena *A, const float *d_xyz, int64_t n, hipStream_t st, float lo[3], float hi[3], int64_t *nv);
// the 1 % .. 99 % quantiles per axis of a sample of d_xyz (one host round trip; false: a HIP error or a full arena)
bool sample_extent(FilterArena *A, const float *d_xyz, int64_t n, hipStream_t st, float lo[3], float hi[3]);
