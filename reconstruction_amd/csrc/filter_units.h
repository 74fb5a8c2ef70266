// filter_units.h -- what crosses the cloud filter's units: the host steps (k_filter.hip) reach the pixel-window search (k_filter_win.hip)
// and the grid and whole-cloud searches (k_filter_knn.hip) through these launchers.  (The units are compiled without relocatable device
// code: a kernel stays in the unit that launches it.)  The filter's public entries are rsm_dev.h's.
#pragma once

#include "cloud_grid.h"
#include "win_bound.h"

// ---- k_filter_win.hip: the lattice copy and the four forms of the pixel-window search
WinGeom win_geom(const FilterLattice &L);
void launch_cloud_lattice(const FilterLattice &L, const WinGeom &g, int64_t n, float4 *lat, unsigned int *cell_of, hipStream_t st);
// the window pass over the whole lattice: dist / undecided (one entry per cloud point; undecided pre-set to 1 by the caller);
// tile_step > 1 + probe_cnt: the sparse probe (see k_sor_window)
void launch_sor_window(const float4 *lat, const WinGeom &g, int mean_k, int radius, float *dist, unsigned int *undecided, hipStream_t st, int tile_step = 1,
                       unsigned int *probe_cnt = nullptr);
// the list form over nq listed queries at radius 24 or 40: dist (per point) / undecided (per list entry)
void launch_sor_window_list(const float4 *lat, const unsigned int *cell_of, const WinGeom &g, int mean_k, int radius, const unsigned int *list, int nq, float *dist,
                            unsigned int *undecided, hipStream_t st);
// the wave form over nq listed queries at any radius -- four waves per query (k_sor_window_wg) while nq <= wg_max: dist (per point) /
// undecided (per list entry)
void launch_sor_window_wave(const float4 *lat, const unsigned int *cell_of, const WinGeom &g, int mean_k, int radius, const unsigned int *list, int nq, float *dist,
                            unsigned int *undecided, hipStream_t st, int wg_max);

// ---- k_filter_outrem.hip: the radius outlier pass's neighbour count on either structure, and its verdict
// the nv finite points of grid G (cell edge = the search radius): count[position in the gridded cloud] = min(#{fdist2 < r2}, cap)
void launch_radius_count_grid(const FilterGridDev &G, int nv, float r2, int cap, int32_t *count, hipStream_t st);
// the m points kept_index lists, on the lattice copy (which holds exactly the finite ones of them): count[o] likewise; points without a
// lattice entry are left as they are
void launch_radius_count_lattice(const float4 *lat, const unsigned int *cell_of, const int32_t *kept_index, int64_t m, const WinGeom &g, double r, float r2,
                                 int cap, int32_t *count, hipStream_t st);
// flag[i] (1 = point i is the pos[i]-th of the counted cloud) &= count[pos[i]] > min_neighbors
void launch_outrem_flags(const int32_t *count, const unsigned int *pos, int64_t n, int min_neighbors, unsigned int *flag, hipStream_t st);

// ---- k_filter_knn.hip: a grid level's search and the whole-cloud search
// nq queries against the 27 cells of grid G (search radius h): d_dist (per point) / undecided (per query: 1 = retry on a coarser grid)
void launch_knn(const float *d_xyz, const FilterGridDev &G, int nv, float h, int mean_k, const unsigned int *queries, int nq, float *d_dist,
                unsigned int *undecided, hipStream_t st);
#define XQ_BATCH 2048 // queries per round of the whole-cloud search (their histograms: 16 MB)
struct XqState { // per listed query
    unsigned int prefix, mask;
    int rank;
    int less;
    double sum;
    unsigned int min_m1; // knn_sum_exact's: the smallest positive squared distance below tau, minus one
};
// cnt <= XQ_BATCH listed queries against the arr_n entries of arr (every finite point once; NaN entries: none); d_xq: XQ_BATCH states,
// d_hist: XQ_BATCH x 2048 ints, zero on entry and on return
void launch_xq_search(const float *d_xyz, const float4 *arr, int arr_n, const unsigned int *list, int cnt, XqState *d_xq, int *d_hist, int mean_k, int nv,
                      float *d_dist, hipStream_t st);
