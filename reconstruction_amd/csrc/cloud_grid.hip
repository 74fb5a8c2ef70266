// cloud_grid.hip -- what the cloud steps (k_filter.hip, k_mls.hip, k_dedup.hip) stand on: the scratch arena's functions (cloud_arena.h)
// and the uniform grid of cloud_grid.h -- the exact bounding box, the robust extent of a sample, and the sort of the points by cell key
// with its cell table.
#include "../../include/rsm.h"
#include "cloud_grid.h"

#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#define FILTER_MAX_CELLS (1 << 25) // most cells a per-cell table is made for (256 MB); beyond that: per-row table / binary search on the keys
// ... for an n-point cloud: a table of far more cells than points is mostly empty, and its bytes are pinned in the context's
// grow-only arena (a 1-point cloud must not cost 256 MB)
static inline size_t filter_max_cells(int64_t n) {
    return (size_t)std::min<int64_t>(FILTER_MAX_CELLS, std::max<int64_t>(1 << 16, 8 * n));
}

__global__ void k_cell_keys(const float *__restrict__ xyz, int64_t n, FGrid g, unsigned long long *__restrict__ keys,
                            unsigned int *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    vals[i] = (unsigned int)i;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) { // PCL's searches skip such points: they sort behind every cell
        keys[i] = ~0ull;
        return;
    }
    int ix, iy, iz;
    grid_cell(g, x, y, z, ix, iy, iz);
    keys[i] = ((unsigned long long)iz * g.ny + iy) * g.nx + ix;
}

__global__ void k_gather_sorted(const float *__restrict__ xyz, const unsigned int *__restrict__ vals, int64_t n,
                                float4 *__restrict__ sxyz) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned int i = vals[j];
    sxyz[j] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __uint_as_float(i));
}

// cell table: (first, one-past-last) sorted index of every cell's points; (0, 0) for an empty cell
// div = 1: per cell; div = nx: per (y, z) row of cells (a deep or thick cloud has too many cells for a table of them)
__global__ void k_cell_table(const unsigned long long *__restrict__ keys, int nv, unsigned long long div, int2 *__restrict__ table) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nv) return;
    const unsigned long long k = keys[i] / div;
    if (i == 0 || keys[i - 1] / div != k) table[k].x = i;
    if (i == nv - 1 || keys[i + 1] / div != k) table[k].y = i + 1;
}

// every `step`-th point into a small buffer (the robust extent's sample)
__global__ void k_sample_points(const float *__restrict__ xyz, int64_t step, int S, float *__restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const size_t i = (size_t)s * (size_t)step;
    out[3 * s] = xyz[3 * i];
    out[3 * s + 1] = xyz[3 * i + 1];
    out[3 * s + 2] = xyz[3 * i + 2];
}

__global__ void k_bbox(const float *__restrict__ xyz, int64_t n, unsigned int *__restrict__ bb) {
    unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    unsigned int nfin = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (!(isfinite(xyz[3 * i]) && isfinite(xyz[3 * i + 1]) && isfinite(xyz[3 * i + 2]))) continue;
        nfin++;
        for (int a = 0; a < 3; a++) {
            const unsigned int o = f2ord(xyz[3 * i + a]);
            lo[a] = min(lo[a], o);
            hi[a] = max(hi[a], o);
        }
    }
    // one set of atomics per WORKGROUP (same-address atomics retire at ~88 per microsecond: per wave they were the kernel)
    __shared__ unsigned int s_r[4][7];
    for (int o = 32; o > 0; o >>= 1) nfin += (unsigned int)__shfl_xor((int)nfin, o);
    for (int a = 0; a < 3; a++)
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], (unsigned int)__shfl_xor((int)lo[a], o));
            hi[a] = max(hi[a], (unsigned int)__shfl_xor((int)hi[a], o));
        }
    if ((threadIdx.x & 63) == 0) {
        unsigned int *r = s_r[threadIdx.x >> 6];
        r[0] = lo[0], r[1] = lo[1], r[2] = lo[2], r[3] = hi[0], r[4] = hi[1], r[5] = hi[2], r[6] = nfin;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int a = threadIdx.x;
        unsigned int v = s_r[0][a];
        for (int w = 1; w < (int)(blockDim.x >> 6); w++) v = a < 3 ? min(v, s_r[w][a]) : (a < 6 ? max(v, s_r[w][a]) : v + s_r[w][a]);
        if (a < 3) atomicMin(&bb[a], v);
        else if (a < 6) atomicMax(&bb[a], v);
        else if (v) atomicAdd(&bb[6], v);
    }
}

// ------------------------------------------------------------------------------------------------ the arena
FilterArena *filter_arena_create() { return new FilterArena(); }
void filter_arena_destroy(FilterArena *a) {
    if (!a) return;
    if (a->base) (void)hipFree(a->base);
    if (a->pin) (void)hipHostFree(a->pin);
    delete a;
}
// room for `bytes` from offset 0 (contents are scratch: nothing survives a call)
int filter_arena_reserve(FilterArena *a, size_t bytes) {
    if (!a->pin && hipHostMalloc((void **)&a->pin, sizeof(FilterPinned), hipHostMallocDefault) != hipSuccess) return RSM_E_NOMEM;
    a->off = 0;
    a->failed = false;
    if (bytes <= a->cap) return RSM_OK;
    // grows geometrically: hipFree synchronises the whole device, other contexts' pairs in flight included
    const size_t want = std::max(bytes, a->cap + a->cap / 2);
    if (a->base) (void)hipFree(a->base);
    a->base = nullptr;
    a->cap = 0;
    if (hipMalloc((void **)&a->base, want) == hipSuccess) a->cap = want;
    else if (hipMalloc((void **)&a->base, bytes) == hipSuccess) a->cap = bytes;
    else return RSM_E_NOMEM;
    return RSM_OK;
}
size_t filter_arena_bytes(int64_t n) { // upper bound of one filter call's scratch for an n-point cloud (callers add their own buffers)
    return (size_t)n * 112 + (filter_max_cells(n) + 64) * sizeof(int2) + std::min<size_t>((size_t)64 << 20, ((size_t)32 << 20) + (size_t)n * 16) /* sort / scan temporaries, the exhaustive search's 16 MB of histograms */;
}
void *filter_arena_alloc(FilterArena *a, size_t bytes) { return a->get<char>(bytes); }
void *filter_arena_host(FilterArena *a) { return a->pin ? a->pin->caller : nullptr; } // (64 bytes of the pinned block that no cloud step uses itself: free for the caller)

// ------------------------------------------------------------------------------------------------ the grid
// robust grid: extents from the 1 % .. 99 % quantiles of a sample (far outliers must not set the cell size)
bool sample_extent(FilterArena *A, const float *d_xyz, int64_t n, hipStream_t st, float lo[3], float hi[3]) {
    const int S = (int)std::min<int64_t>(n, FA_SAMPLES);
    const size_t mark = A->off;
    float *d_s = A->get<float>((size_t)3 * S);
    float *h = A->pin->samples;
    if (!d_s) return false;
    hipLaunchKernelGGL(k_sample_points, blocks_for(S), dim3(256), 0, st, d_xyz, n / S, S, d_s);
    if (hipMemcpyAsync(h, d_s, sizeof(float) * 3 * (size_t)S, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return false;
    A->off = mark;
    for (int a = 0; a < 3; a++) {
        std::vector<float> v;
        for (int s = 0; s < S; s++)
            if (std::isfinite(h[3 * (size_t)s]) && std::isfinite(h[3 * (size_t)s + 1]) && std::isfinite(h[3 * (size_t)s + 2])) v.push_back(h[3 * (size_t)s + a]);
        if (v.empty()) v.push_back(0.0f);
        const size_t q_lo = (size_t)(0.01 * (v.size() - 1)), q_hi = (size_t)(0.99 * (v.size() - 1)); // (two selections: a full sort of the
        std::nth_element(v.begin(), v.begin() + q_lo, v.end());                                        // three samples took 0.8 ms of every call)
        lo[a] = v[q_lo];
        std::nth_element(v.begin() + q_lo, v.begin() + q_hi, v.end());
        hi[a] = v[q_hi];
    }
    return true;
}

int build_grid(FilterArena *A, const float *d_xyz, int64_t n, int64_t nv, float h, const float bb_lo[3], const float bb_hi[3], hipStream_t st,
               FilterGridDev &G) {
    const double H = grid_edge(h);
    G.g.inv_h = 1.0 / H;
    auto dim = [&](int a) { return (int)std::min<double>(1 << 20, std::max<double>(1.0, floor(((double)bb_hi[a] - (double)bb_lo[a]) / H) + 1.0)); };
    int ax[3] = {0, 1, 2};
    std::sort(ax, ax + 3, [&](int a, int b) { return dim(a) != dim(b) ? dim(a) > dim(b) : a < b; }); // most cells first = fastest key digit
    G.g.p0 = ax[0], G.g.p1 = ax[1], G.g.p2 = ax[2];
    G.g.ox = (double)bb_lo[ax[0]], G.g.oy = (double)bb_lo[ax[1]], G.g.oz = (double)bb_lo[ax[2]];
    G.g.nx = dim(ax[0]), G.g.ny = dim(ax[1]), G.g.nz = dim(ax[2]);
    unsigned long long *k1 = A->get<unsigned long long>((size_t)n), *k2 = A->get<unsigned long long>((size_t)n);
    unsigned int *v1 = A->get<unsigned int>((size_t)n), *v2 = A->get<unsigned int>((size_t)n);
    G.sxyz = A->get<float4>((size_t)n);
    if (!k1 || !k2 || !v1 || !v2 || !G.sxyz) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_cell_keys, blocks_for(n), dim3(256), 0, st, d_xyz, n, G.g, k1, v1);
    const int s = sort_pairs(*A, k1, k2, v1, v2, (size_t)n, 64 /* non-finite points carry the key ~0: all bits take part */, st);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL(k_gather_sorted, blocks_for(n), dim3(256), 0, st, d_xyz, v2, n, G.sxyz);
    G.keys = k2;
    G.vals = v2;
    G.table = nullptr;
    G.table_kind = 0;
    const double ncell = (double)G.g.nx * G.g.ny * G.g.nz, nrow = (double)G.g.ny * G.g.nz;
    const double max_cells = (double)filter_max_cells(n);
    if (nv > 0 && (ncell <= max_cells || nrow <= max_cells)) {
        G.table_kind = ncell <= max_cells ? 1 : 2;
        const size_t nc = (size_t)(G.table_kind == 1 ? ncell : nrow);
        G.table = A->get<int2>(nc);
        if (!G.table) return RSM_E_NOMEM;
        DEVCHK(hipMemsetAsync(G.table, 0, sizeof(int2) * nc, st));
        hipLaunchKernelGGL(k_cell_table, blocks_for(nv), dim3(256), 0, st, k2, (int)nv, (unsigned long long)(G.table_kind == 1 ? 1 : G.g.nx), G.table);
    }
    return RSM_OK;
}

int cloud_bbox(FilterArena *A, const float *d_xyz, int64_t n, hipStream_t st, float lo[3], float hi[3], int64_t *nv) {
    *nv = 0;
    for (int a = 0; a < 3; a++) lo[a] = hi[a] = 0.0f;
    if (n <= 0) return RSM_OK;
    if (!A->pin) return RSM_E_STATE;
    unsigned int *d_bb = A->get<unsigned int>(8);
    if (!d_bb) return RSM_E_NOMEM;
    unsigned int *h_bb = A->pin->bb;
    const unsigned int init[7] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u, 0u};
    memcpy(h_bb, init, sizeof init);
    DEVCHK(hipMemcpyAsync(d_bb, h_bb, sizeof init, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bbox, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, st, d_xyz, n, d_bb);
    DEVCHK(hipMemcpyAsync(h_bb, d_bb, sizeof init, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    *nv = h_bb[6];
    for (int a = 0; a < 3 && *nv; a++) {
        lo[a] = ord2f(h_bb[a]);
        hi[a] = ord2f(h_bb[3 + a]);
    }
    return RSM_OK;
}
