// k_poisson_band.hip -- the Poisson surface one level finer than the dense grid reaches (script1.mlx's OctDepth 10): a finest
// level of N = 2^depth nodes per axis that exists only near the samples, on top of k_poisson.hip's dense solve at depth - 1.  The fine grid
// is cut into bricks of 8^3 nodes; a brick is occupied when a sample's cell lies in it and active within band_bricks (Chebyshev) of an
// occupied one.  The active bricks are listed in ascending linear index, a brick's slot is its place in the list, a dense B^3 table maps
// brick -> slot (-1: inactive), and every field lives brick-major: element slot * 512 + lx + 8 (ly + 8 lz).  Splat, right-hand side, chi at
// the samples and the extraction are the rules DESIGN.md 9 f42 states once (poisson_space.h, poisson_common.h), here on the
// BandSpace; what is this file's own (restated in numpy in tests/poisson_band_restatement.py):
//   bricks   occupied -> dilated -> scan -> slot table, list, the 27 neighbour slots of every slot     k_pb_mark .. k_pb_nbr
//   guess    g = (float)(1/4 trilinear prolongation of the coarse chi), fp64, corner order dz, dy, dx  k_pb_guess
//   solve    L chi = b on the active nodes, chi = g on the inactive ones, 0 outside the grid: float32 conjugate gradients from chi = g,
//            preconditioned by one symmetric red-black Gauss-Seidel sweep from zero on the band        k_pb_rbgs, k_pb_stencil
//   trim     f7's trim with the occupancy dilated inside the band                                      k_pb_dilate_cells
// One workgroup per brick in the solver: a 10^3 tile of the field in LDS, filled through the slot's neighbour table.  Every reduction has a fixed
// shape: an LDS tree over a brick's 512 products, the per-slot partials through f7's tree (poisson_tree_sum).  No float atomics.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"
#include "poisson_common.h"

#include <math.h>

// the band solve ends after this many iterations in a row without a new best residual (twice the longest such run of the
// restatement's float32 histories before their floor)
#define PB_STALL 20

namespace {

// ---- bricks ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pb_mark(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, MtGrid g, int bsh,
                                                 uint8_t *__restrict__ occb) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double p[3], nh[3];
    if (!pv_valid(xyz, nrm, s, p, nh)) return;
    const double o[3] = {g.ox, g.oy, g.oz};
    int c[3];
    for (int a = 0; a < 3; a++) {
        const int cc = (int)floor((p[a] - o[a]) / g.h);
        c[a] = (cc < 0 ? 0 : (cc > g.N - 1 ? g.N - 1 : cc)) >> 3;
    }
    occb[(size_t)c[0] + (((size_t)c[1] + ((size_t)c[2] << bsh)) << bsh)] = 1;
}
struct PbU8ToU32 {
    __host__ __device__ unsigned int operator()(uint8_t v) const { return v ? 1u : 0u; }
};
__global__ __launch_bounds__(256) void k_pb_slots(const uint8_t *__restrict__ act, const unsigned int *__restrict__ pos, size_t B3, int32_t *__restrict__ slot,
                                                  int32_t *__restrict__ active) {
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B3) return;
    slot[b] = act[b] ? (int32_t)pos[b] : -1;
    if (act[b] && active) active[pos[b]] = (int32_t)b;
}
// the slot table from a caller's list
__global__ __launch_bounds__(256) void k_pb_slots_of_list(const int32_t *__restrict__ active, int S, int32_t *__restrict__ slot) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < S) slot[active[s]] = s;
}
__global__ __launch_bounds__(256) void k_pb_nbr(const int32_t *__restrict__ active, int S, const int32_t *__restrict__ slot, int bsh, int32_t *__restrict__ nbr) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)S * 27) return;
    const int s = (int)(t / 27), code = (int)(t % 27);
    const int B = 1 << bsh, b = active[s];
    const int x = (b & (B - 1)) + code % 3 - 1, y = ((b >> bsh) & (B - 1)) + (code / 3) % 3 - 1, z = (b >> (2 * bsh)) + code / 9 - 1;
    nbr[t] = (x < 0 || y < 0 || z < 0 || x >= B || y >= B || z >= B) ? -2 : slot[(size_t)x + (((size_t)y + ((size_t)z << bsh)) << bsh)];
}

// ---- splat (f7's step 3 on the active nodes; the right-hand side is poisson_space.h's k_pv_rhs) ------------------------------------------------
__global__ __launch_bounds__(256) void k_pb_splat(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, MtGrid g, BandSpace S,
                                                  unsigned long long *__restrict__ V /* [3][S 512] */, uint8_t *__restrict__ occ) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double p[3], nh[3];
    if (!pv_valid(xyz, nrm, s, p, nh)) return;
    int c[3];
    pv_occ_cell3(p, g, c);
    const long long ce = S.elem(c[0], c[1], c[2]);
    if (ce >= 0) occ[ce] = 1; // (the cell's brick is occupied, so active)
    pv_splat8(S, p, g, nh, V, S.nodes());
}

// ---- guess: a quarter of the cell-centred trilinear prolongation of the coarse field (chi_c = 0 outside its grid) -------------------------------
__device__ __forceinline__ float pb_guess(const float *__restrict__ chic, int shc, int i, int j, int k) {
    const int Nc = 1 << shc, c[3] = {i, j, k};
    int i0[3];
    double f[3];
    for (int a = 0; a < 3; a++) {
        i0[a] = (c[a] - 1) >> 1; // the lower of the two coarse nodes: the parent of an odd fine node, the parent's lower neighbour of an even one
        f[a] = (c[a] & 1) ? 0.25 : 0.75;
    }
    double acc = 0.0;
    for (int dz = 0; dz < 2; dz++)
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const int x = i0[0] + dx, y = i0[1] + dy, z = i0[2] + dz;
                if (x < 0 || y < 0 || z < 0 || x >= Nc || y >= Nc || z >= Nc) continue;
                const double w = ((dx ? f[0] : 1.0 - f[0]) * (dy ? f[1] : 1.0 - f[1])) * (dz ? f[2] : 1.0 - f[2]);
                acc += w * (double)chic[(size_t)x + (((size_t)y + ((size_t)z << shc)) << shc)];
            }
    return (float)(0.25 * acc);
}
__global__ __launch_bounds__(256) void k_pb_guess(const float *__restrict__ chic, PbBand B, size_t nodes, float *__restrict__ g) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nodes) return;
    int o[3];
    pb_origin(B, (int)(t >> 9), o);
    const int l = (int)(t & 511);
    g[t] = pb_guess(chic, B.sh - 1, o[0] + (l & 7), o[1] + ((l >> 3) & 7), o[2] + (l >> 6));
}

// ---- the band solve: one workgroup of 256 threads per brick ----------------------------------------------------------------------------------
// the sum of a brick's 512 products (thread t gives those of nodes t and t + 256) by a fixed LDS tree -> *dst
__device__ __forceinline__ void pb_brick_sum_to(double a, double b, double *dst) {
    __shared__ double s[PB_NODES];
    s[threadIdx.x] = a;
    s[threadIdx.x + 256] = b;
    __syncthreads();
    for (int w = 256; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = s[0];
}
// the 10^3 tile of x around the brick of `slot`: tile[(x + 1) + 10 ((y + 1) + 10 (z + 1))].  GUESS: an inactive node inside the grid holds the guess
// there (chi = g + e with e = 0; no coarse field: 0); otherwise, and outside the grid, 0
template <bool GUESS>
__device__ __forceinline__ void pb_fill_tile(float *tile, int32_t *nb, const float *__restrict__ x, const PbBand &B, int slot, const float *__restrict__ chic) {
    if (threadIdx.x < 27) nb[threadIdx.x] = B.nbr[(size_t)slot * 27 + threadIdx.x];
    __syncthreads();
    int o[3] = {0, 0, 0};
    if (GUESS) pb_origin(B, slot, o);
    for (int t = threadIdx.x; t < 1000; t += 256) {
        const int lx = t % 10 - 1, ly = (t / 10) % 10 - 1, lz = t / 100 - 1;
        const long long e = pb_node(nb, lx, ly, lz);
        float v = 0.0f;
        if (e >= 0) v = x[e];
        else if (GUESS && e == -1 && chic) v = pb_guess(chic, B.sh - 1, o[0] + lx, o[1] + ly, o[2] + lz);
        tile[t] = v;
    }
    __syncthreads();
}
__device__ __forceinline__ float pb_tile_nbr_sum(const float *tile, int c) { // c = the node's place in the tile; f7's order of additions
    return ((tile[c - 1] + tile[c + 1]) + (tile[c - 10] + tile[c + 10])) + (tile[c - 100] + tile[c + 100]);
}
// MODE 0: out = L x (x = 0 off the band), partials of x . out;  1: out = b - L x (x = the guess off the band), partials of out^2
template <int MODE>
__global__ __launch_bounds__(256) void k_pb_stencil(const float *__restrict__ x, const float *__restrict__ b, float *__restrict__ out, PbBand B,
                                                    const float *__restrict__ chic, double *__restrict__ part) {
    __shared__ float tile[1000];
    __shared__ int32_t nb[27];
    const int slot = blockIdx.x;
    pb_fill_tile<MODE == 1>(tile, nb, x, B, slot, chic);
    double acc[2];
    for (int h = 0; h < 2; h++) {
        const int l = threadIdx.x + 256 * h;
        const int c = ((l & 7) + 1) + 10 * ((((l >> 3) & 7) + 1) + 10 * ((l >> 6) + 1));
        const size_t e = (size_t)slot * PB_NODES + l;
        const float v = tile[c];
        const float lx = pb_tile_nbr_sum(tile, c) - 6.0f * v;
        if (MODE == 0) {
            out[e] = lx;
            acc[h] = (double)v * (double)lx;
        } else {
            const float r = b[e] - lx;
            out[e] = r;
            acc[h] = (double)r * (double)r;
        }
    }
    pb_brick_sum_to(acc[0], acc[1], &part[slot]);
}
// one colour of a red-black Gauss-Seidel sweep on the band (x = 0 off it): x = (sum of neighbours - b) / 6 where (i + j + k) & 1 == colour (a
// brick's origin is even, so the local parity is the global one).  FIRST: the sweep's first pass from x = 0, which also writes the zeros of
// the other colour.  part (optional): partials of b . x after the pass
template <bool FIRST>
__global__ __launch_bounds__(256) void k_pb_rbgs(float *__restrict__ x, const float *__restrict__ b, PbBand B, int colour, double *__restrict__ part) {
    __shared__ float tile[1000];
    __shared__ int32_t nb[27];
    const int slot = blockIdx.x;
    if (!FIRST) pb_fill_tile<false>(tile, nb, x, B, slot, nullptr);
    const int ly = (threadIdx.x >> 2) & 7, lz = threadIdx.x >> 5;
    const int lx = 2 * (threadIdx.x & 3) + ((ly + lz + colour) & 1);
    const int l = lx + 8 * (ly + 8 * lz), lo = l ^ 1; // lo: the node of the other colour beside it
    const size_t e = (size_t)slot * PB_NODES + l, eo = (size_t)slot * PB_NODES + lo;
    const int c = (lx + 1) + 10 * ((ly + 1) + 10 * (lz + 1));
    const float sum = FIRST ? ((0.0f + 0.0f) + (0.0f + 0.0f)) + (0.0f + 0.0f) : pb_tile_nbr_sum(tile, c);
    const float be = b[e];
    const float v = (sum - be) / 6.0f;
    x[e] = v;
    if (FIRST) x[eo] = 0.0f;
    if (part) {
        const float vo = FIRST ? 0.0f : tile[c + (lo - l)];
        pb_brick_sum_to((double)be * (double)v, (double)b[eo] * (double)vo, &part[slot]);
    }
}
__global__ __launch_bounds__(256) void k_pb_dot(const float *__restrict__ x, const float *__restrict__ y, double *__restrict__ part) {
    const size_t e = (size_t)blockIdx.x * PB_NODES + threadIdx.x;
    pb_brick_sum_to((double)x[e] * (double)y[e], (double)x[e + 256] * (double)y[e + 256], &part[blockIdx.x]);
}
// one axis of the Chebyshev dilation of the cells' occupancy inside the band (0 off it)
__global__ __launch_bounds__(256) void k_pb_dilate_cells(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, PbBand B, size_t nodes, int axis, int r) {
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= nodes) return;
    int p[3];
    pb_origin(B, (int)(a >> 9), p);
    const int l = (int)(a & 511);
    p[0] += l & 7;
    p[1] += (l >> 3) & 7;
    p[2] += l >> 6;
    const int c = p[axis];
    const int lo = c - r < 0 ? 0 : c - r, hi = c + r > B.N - 1 ? B.N - 1 : c + r;
    uint8_t m = 0;
    for (int q = lo; q <= hi && !m; q++) {
        p[axis] = q;
        const long long e = pb_elem_of(B, p[0], p[1], p[2]);
        m = (e >= 0 && in[e]) ? 1 : 0;
    }
    out[a] = m;
}

} // namespace

void poisson_band_free(PoissonBand *b) {
    if (!b) return;
    for (int32_t *p : {b->d_slot, b->d_active, b->d_nbr})
        if (p) (void)hipFree(p);
    b->d_slot = b->d_active = b->d_nbr = nullptr;
    b->n_active = b->n_occupied = 0;
}

// the list and the neighbour table of a band whose slot table and count are there
static int pb_finish_tables(PoissonBand *out, hipStream_t st) {
    const int bsh = out->depth - 3;
    hipLaunchKernelGGL(k_pb_nbr, blocks_for((size_t)out->n_active * 27), dim3(256), 0, st, (const int32_t *)out->d_active, (int)out->n_active,
                       (const int32_t *)out->d_slot, bsh, out->d_nbr);
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    return RSM_OK;
}

int poisson_band_bricks_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, const double grid[4], int band_bricks, int64_t max_bricks,
                               PoissonBand *out, hipStream_t st) {
    poisson_band_free(out);
    out->depth = depth;
    const int bsh = depth - 3;
    const size_t B3 = (size_t)1 << (3 * bsh);
    DevMem M;
    uint8_t *t0 = M.get<uint8_t>(B3), *t1 = M.get<uint8_t>(B3);
    unsigned int *pos = M.get<unsigned int>(B3), *opos = M.get<unsigned int>(B3);
    if (!M.ok || hipMalloc((void **)&out->d_slot, B3 * sizeof(int32_t)) != hipSuccess) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(t0, 0, B3, st));
    hipLaunchKernelGGL(k_pb_mark, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, pv_grid(grid, depth), bsh, t0);
    int s = scan_u32(M, rocprim::make_transform_iterator((const uint8_t *)t0, PbU8ToU32()), opos, B3, st);
    if (s != RSM_OK) return s;
    uint64_t nocc = 0, nact = 0;
    if ((s = scan_total(t0, opos, B3, st, &nocc)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_pv_dilate<>, blocks_for(B3), dim3(256), 0, st, (const uint8_t *)t0, t1, bsh, 0, band_bricks);
    hipLaunchKernelGGL(k_pv_dilate<>, blocks_for(B3), dim3(256), 0, st, (const uint8_t *)t1, t0, bsh, 1, band_bricks);
    hipLaunchKernelGGL(k_pv_dilate<>, blocks_for(B3), dim3(256), 0, st, (const uint8_t *)t0, t1, bsh, 2, band_bricks);
    if ((s = scan_u32(M, rocprim::make_transform_iterator((const uint8_t *)t1, PbU8ToU32()), pos, B3, st)) != RSM_OK) return s;
    if ((s = scan_total(t1, pos, B3, st, &nact)) != RSM_OK) return s;
    DEVCHK(hipGetLastError());
    out->n_occupied = (int64_t)nocc;
    out->n_active = (int64_t)nact;
    if (nact == 0 || (int64_t)nact > max_bricks) return RSM_OK; // (the caller refuses a band above its cap by name)
    if (hipMalloc((void **)&out->d_active, nact * sizeof(int32_t)) != hipSuccess || hipMalloc((void **)&out->d_nbr, nact * 27 * sizeof(int32_t)) != hipSuccess)
        return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_pb_slots, blocks_for(B3), dim3(256), 0, st, (const uint8_t *)t1, (const unsigned int *)pos, B3, out->d_slot, out->d_active);
    return pb_finish_tables(out, st);
}

int poisson_band_of_list_device(const int32_t *h_bricks, int64_t n_bricks, int depth, PoissonBand *out, hipStream_t st) {
    poisson_band_free(out);
    out->depth = depth;
    const size_t B3 = (size_t)1 << (3 * (depth - 3));
    if (hipMalloc((void **)&out->d_slot, B3 * sizeof(int32_t)) != hipSuccess) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(out->d_slot, 0xff, B3 * sizeof(int32_t), st)); // -1
    out->n_active = n_bricks;
    if (n_bricks == 0) return mesh_finish(st);
    if (hipMalloc((void **)&out->d_active, (size_t)n_bricks * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void **)&out->d_nbr, (size_t)n_bricks * 27 * sizeof(int32_t)) != hipSuccess)
        return RSM_E_NOMEM;
    DEVCHK(hipMemcpyAsync(out->d_active, h_bricks, (size_t)n_bricks * sizeof(int32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pb_slots_of_list, blocks_for((size_t)n_bricks), dim3(256), 0, st, (const int32_t *)out->d_active, (int)n_bricks, out->d_slot);
    return pb_finish_tables(out, st);
}

int poisson_band_rhs_device(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, const double grid[4], float *d_b32, double *d_b64,
                            uint8_t *d_occ, hipStream_t st) {
    const size_t nodes = pb_nodes(band);
    DevMem M;
    unsigned long long *V = M.get<unsigned long long>(3 * nodes);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(V, 0, 3 * nodes * sizeof(unsigned long long), st));
    DEVCHK(hipMemsetAsync(d_occ, 0, nodes, st));
    const BandSpace S = pb_space(band);
    hipLaunchKernelGGL(k_pb_splat, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, pv_grid(grid, band.depth), S, V, d_occ);
    hipLaunchKernelGGL((k_pv_rhs<BandSpace, long long>), blocks_for(nodes), dim3(256), 0, st, (const long long *)V, S, d_b32, d_b64);
    return mesh_finish(st);
}

int poisson_band_guess_device(const PoissonBand &band, const float *d_chi_c, float *d_g, hipStream_t st) {
    const size_t nodes = pb_nodes(band);
    hipLaunchKernelGGL(k_pb_guess, blocks_for(nodes), dim3(256), 0, st, d_chi_c, pb_band(band), nodes, d_g);
    return mesh_finish(st);
}

namespace {
// poisson_pcg's Ops on the band: one symmetric red-black Gauss-Seidel sweep from zero as the preconditioner
struct BandSolver {
    PbBand B;
    unsigned S; // the active bricks
    size_t n;
    const float *rhs, *chi_c;
    float *r, *z;
    double *part, *part2, *scal;
    hipStream_t st;
    int fetch(double *out) { // the sum of the per-slot partials, in slot order through f7's tree
        poisson_tree_sum(part, (int64_t)S, part2, scal, st);
        DEVCHK(hipMemcpyAsync(out, scal, sizeof(double), hipMemcpyDeviceToHost, st));
        DEVCHK(hipStreamSynchronize(st));
        return RSM_OK;
    }
    int precondition(double *rho) { // red, black, (black again would recompute the same values from the same red ones), red; the last pass gives r . z
        hipLaunchKernelGGL(k_pb_rbgs<true>, dim3(S), dim3(256), 0, st, z, (const float *)r, B, 0, (double *)nullptr);
        hipLaunchKernelGGL(k_pb_rbgs<false>, dim3(S), dim3(256), 0, st, z, (const float *)r, B, 1, (double *)nullptr);
        hipLaunchKernelGGL(k_pb_rbgs<false>, dim3(S), dim3(256), 0, st, z, (const float *)r, B, 0, part);
        return fetch(rho);
    }
    int apply(const float *p, float *q, double *pq) {
        hipLaunchKernelGGL(k_pb_stencil<0>, dim3(S), dim3(256), 0, st, p, (const float *)nullptr, q, B, (const float *)nullptr, part);
        return fetch(pq);
    }
    int residual(const float *chi, double *rr) {
        hipLaunchKernelGGL(k_pb_stencil<1>, dim3(S), dim3(256), 0, st, chi, rhs, r, B, chi_c, part);
        return fetch(rr);
    }
};
} // namespace

int poisson_band_solve_device(const PoissonBand &band, const float *d_b, const float *d_chi_c, double rel_residual, int max_iterations, float *d_chi,
                              double *residual0, double *residual, int *iterations, double *history, hipStream_t st) {
    const size_t nodes = pb_nodes(band);
    *residual0 = *residual = 0.0;
    *iterations = 0;
    DevMem M; // (all of the solve's scratch before its first launch)
    BandSolver A{pb_band(band), (unsigned)band.n_active, nodes, d_b, d_chi_c};
    A.r = M.get<float>(nodes), A.z = M.get<float>(nodes);
    float *p = M.get<float>(nodes), *q = M.get<float>(nodes), *best = M.get<float>(nodes);
    A.part = M.get<double>(A.S), A.part2 = M.get<double>(POISSON_SUM_PARTIALS), A.scal = M.get<double>(1);
    A.st = st;
    if (!M.ok) return RSM_E_NOMEM;
    double bb = 0.0, rr = 0.0;
    hipLaunchKernelGGL(k_pb_dot, dim3(A.S), dim3(256), 0, st, d_b, d_b, A.part);
    int s = A.fetch(&bb);
    if (s != RSM_OK) return s;
    if (!(bb > 0.0)) return mesh_finish(st); // b = 0 on the band: chi stays the guess
    const double bnorm = sqrt(bb);
    if ((s = A.residual(d_chi, &rr)) != RSM_OK) return s;
    *residual0 = *residual = sqrt(rr) / bnorm;
    if (*residual > rel_residual) {
        DEVCHK(hipMemcpyAsync(best, d_chi, nodes * sizeof(float), hipMemcpyDeviceToDevice, st));
        if ((s = poisson_pcg(A, bnorm, rel_residual, max_iterations, PB_STALL, d_chi, p, q, best, residual, iterations, history, st)) != RSM_OK) return s;
    }
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    return *residual <= rel_residual ? RSM_OK : RSM_W_NOT_CONVERGED;
}

void poisson_band_chi_at_samples(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, const float *d_chi, const double grid[4], double *d_val,
                                 hipStream_t st) {
    hipLaunchKernelGGL(k_pv_chi_at_samples<BandSpace>, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, pv_grid(grid, band.depth), pb_space(band), d_chi, d_val);
}

int poisson_band_iso_device(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, int64_t n_valid, const float *d_chi,
                            const double grid[4], double *iso, hipStream_t st) {
    auto chi_at = [&](double *val) { poisson_band_chi_at_samples(band, d_xyz, d_nrm4, n, d_chi, grid, val, st); };
    return poisson_mean_of_chi_at_samples(chi_at, n, nullptr, (double)n_valid, iso, st);
}

int poisson_band_extract_device(const PoissonBand &band, const float *d_chi, double iso, const double grid[4], const uint8_t *d_occ, int trim_cells,
                                PoissonMesh *out, int64_t untrimmed[2], hipStream_t st) {
    const BandSpace S = pb_space(band);
    auto dilate = [&](const uint8_t *in, uint8_t *to, int axis) {
        hipLaunchKernelGGL(k_pb_dilate_cells, blocks_for(S.nodes()), dim3(256), 0, st, in, to, S.B, S.nodes(), axis, trim_cells);
    };
    return poisson_extract(S, pv_grid(grid, band.depth), d_chi, iso, d_occ, trim_cells, dilate, out, untrimmed, st);
}
