// k_filter_outrem.hip -- the second outlier pass of CCloudOptimization::filter: pcl::RadiusOutlierRemoval between cloud_after_1step and
// cloud_filtered (CloudOptimization/CCloudOptimization.cpp:90-96; parameters outrem_neighbor / outrem_radius, CReconstruction.cpp:18).  The
// reference ships the block commented out; its interface and its per-data-set tunings carry the values.  Restated from PCL 1.7.2's
// RadiusOutlierRemoval::applyFilterIndices as published (parity unpinned), with k_filter.hip's conventions: float32 neighbour distances,
// dist^2 < r^2.
//   S = the survivors of the outlier removal before it, in order; S_f its finite points.
//   count(p) = #{ q in S_f : fdist2(p, q) < r2 },  r2 = (float)(radius * radius): the point itself counts (radiusSearch returns the query),
//   coincident points count once each, a non-finite p has count 0.  p stays iff count(p) > min_neighbors.
// Only that comparison matters to the filter, so a count stops at cap = min_neighbors + 1; rsm_stage_radius_count shows the stop as
// count = min(count(p), cap).
// The count is the normals' radius search with an integer in place of the nine sums, on the same two structures: the grid of radius-cells
// (cloud_grid.h: 27 cells = 9 ranges of the sorted array) and the pixel lattice of a depth-map cloud (win_bound.h: win_need).
// The stop is per lane: the loop's condition carries `cnt < cap`, a lane that has its answer is masked off and issues no more loads, and
// the wave leaves a loop when its last lane does -- which is what a wave-wide vote would compute, without the vote.  No LDS, no atomics.
#include "filter_units.h"

// thread = a point of the sorted array (the finite ones: the others sort behind them and keep the count the buffer is filled with);
// the count goes to the point's position in S
__global__ __launch_bounds__(256) void k_radius_count_grid(const float4 *__restrict__ sxyz, const unsigned long long *__restrict__ keys, int n, FGrid g, float r2,
                                                            int cap, int32_t *__restrict__ count) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const float4 p = sxyz[j];
    int ix, iy, iz;
    grid_cell(g, p.x, p.y, p.z, ix, iy, iz);
    int cnt = 0;
    for (int t = 0; t < 9 && cnt < cap; t++) { // ranges9's ranges, each found when the walk reaches it: no array of them, no scratch
        int rs, re;
        range_of9(keys, n, g, ix, iy, iz, t, rs, re);
        for (int q = rs; q < re && cnt < cap; q++) {
            const float4 o = sxyz[q];
            cnt += fdist2(p.x, p.y, p.z, o.x, o.y, o.z) < r2;
        }
    }
    count[__float_as_uint(p.w)] = cnt;
}

// thread = a point of S; the lattice copy holds S_f (the points the pass before removed are blanked).  One window per wave, as in
// k_normals_lattice: the largest any of its points needs for the radius r, at most WIN_PAD (the copy's border: no bounds checks).
__global__ __launch_bounds__(256) void k_radius_count_lattice(const float4 *__restrict__ lat, const unsigned int *__restrict__ cell_of,
                                                               const int32_t *__restrict__ kept_index, int64_t m, WinGeom g, double r, float r2, int cap,
                                                               int32_t *__restrict__ count) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float4 p = make_float4(__uint_as_float(0x7fc00000u), 0.0f, 0.0f, 0.0f);
    unsigned int cell = 0;
    if (o < m) {
        cell = cell_of[kept_index[o]];
        p = lat[cell];
    }
    const bool live = p.x == p.x; // (a non-finite point has no lattice entry: count 0, the buffer's fill)
    int w = live ? win_need(p, g, r) : 0;
    for (int t = 32; t > 0; t >>= 1) w = max(w, __shfl_xor(w, t));
    w = min(w, WIN_PAD);
    if (!live) return;
    int cnt = 0;
    for (int b = -w; b <= w && cnt < cap; b++) {
        const float4 *row = lat + (size_t)cell + (ptrdiff_t)b * g.gw;
        for (int a = -w; a <= w && cnt < cap; a++) {
            const float4 q = row[a];
            cnt += fdist2(p.x, p.y, p.z, q.x, q.y, q.z) < r2; // (NaN: a pixel without a point, or a removed one)
        }
    }
    count[o] = cnt;
}

// flag (per point of the unfiltered cloud: 1 = in S, pos = its place there) becomes "survives both passes"
__global__ void k_outrem_flags(const int32_t *__restrict__ count, const unsigned int *__restrict__ pos, int64_t n, int min_neighbors,
                               unsigned int *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) flag[i] = count[pos[i]] > min_neighbors; // removed: k <= min_pts_radius_
}

void launch_radius_count_grid(const FilterGridDev &G, int nv, float r2, int cap, int32_t *count, hipStream_t st) {
    if (nv > 0) hipLaunchKernelGGL(k_radius_count_grid, blocks_for(nv), dim3(256), 0, st, G.sxyz, G.keys, nv, G.g, r2, cap, count);
}
void launch_radius_count_lattice(const float4 *lat, const unsigned int *cell_of, const int32_t *kept_index, int64_t m, const WinGeom &g, double r, float r2,
                                 int cap, int32_t *count, hipStream_t st) {
    if (m > 0) hipLaunchKernelGGL(k_radius_count_lattice, blocks_for(m), dim3(256), 0, st, lat, cell_of, kept_index, m, g, r, r2, cap, count);
}
void launch_outrem_flags(const int32_t *count, const unsigned int *pos, int64_t n, int min_neighbors, unsigned int *flag, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_outrem_flags, blocks_for(n), dim3(256), 0, st, count, pos, n, min_neighbors, flag);
}
