// k_poisson_density.hip -- the density-adaptive form of the Poisson surface's splat, where mesh.bat runs PoissonRecon --samplesPerNode 2 and
// script1.mlx sets SamplesPerNode 3: a sample in a thinly sampled region is spread over a coarser level of the grid and weighs more, so that the
// surface does not cave in where the cloud is thin.  Not a bit-parity port of that tool (no source in the reference tree): every rule is
// defined in DESIGN.md 9 (f14) and restated in numpy in tests/poisson_density_restatement.py.
//   density      rho_s = f11's count splat on 2^kernel_depth nodes per axis, read back at the sample's own position; value_s = f11's value.
//                k_meshtrim.hip's own kernels through density_at_points_device (mesh_common.h): stated there, called here
//   sample pass  w_s = min(1, 1 / (64 rho_s)), d_s = min(depth, max(3, value_s or the caller's depth)); the least d_s, how many lie
//                below depth                                                                                            k_pd_sample
//   level splat  at level lo = floor(d_s) with alpha = (1 - fr) w_s and, below depth, at lo + 1 with alpha = fr w_s (fr = d_s - lo):
//                V_L[a](node) += llrint((wt (alpha n^_a)) 2^32), f7's trilinear weights on the level's 2^L nodes per axis; 64-bit integer
//                atomics, so no order in the sum.  |wt alpha n^_a| <= 1 and a sample meets a node once per level: f7's 2^63 bound holds per
//                level.  occ is f7's, on the finest level                                                                k_pd_splat
//   cascade      U_3 = V_3 2^-32 8^(3 - depth); U_L = V_L 2^-32 8^(L - depth) + P(U_{L-1}) in fp64, in place of V_L; P = cell-centred trilinear
//                prolongation, x then y then z, 0.75 near + 0.25 far, 0 outside                                         k_pd_cascade
//   rhs          f7's central differences of U_depth in fp64, rounded once to float for the solver                     k_pv_rhs<DenseSpace, double>
//   iso          sum w_s chi(p_s) / sum w_s: f7's chi at the samples (poisson_chi_at_samples) times w_s, both sums in f7's tree   k_pd_mul
// The levels share one buffer of 64-bit words: level L's three components start at word 3 (8^L - 8^3) / 7.  The buffer's top level and the
// finest depth are two numbers: the banded call (k_poisson_band_density.hip; f17) keeps the levels 3..depth - 1 here and the finest on its bricks.
// No float atomics.  Built with -ffp-contract=off (csrc/Makefile): every fp64 expression below is evaluated as written.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"
#include "poisson_density_common.h"
#include "poisson_space.h"

#include <math.h>
#include <string.h>

namespace {

typedef unsigned long long u64;

struct PdBox { // f7's grid at the finest level `depth`, and the buffer's top level (<= depth)
    MtGrid g;
    int depth, top;
};
__host__ __device__ __forceinline__ size_t pd_level_nodes(int L) { return (size_t)1 << (3 * L); }
__host__ __device__ __forceinline__ size_t pd_level_word(int L) { return 3 * ((pd_level_nodes(L) - pd_level_nodes(PD_LMIN)) / 7); }
// level L's grid: h_L = side / 2^L = h 2^(depth - L), exact
__device__ __forceinline__ MtGrid pd_level_grid(const PdBox &b, int L) { return MtGrid{b.g.ox, b.g.oy, b.g.oz, b.g.h * (double)(1 << (b.depth - L)), 1 << L}; }

// ---- 3: weight and depth of a sample; ctr[0] = the least d_s as its bit pattern (d_s > 0: the order of the doubles), ctr[1] = samples below depth
__global__ __launch_bounds__(256) void k_pd_sample(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, int depth,
                                                   const double *__restrict__ depth_in, const double *__restrict__ val, double *__restrict__ rho,
                                                   double *__restrict__ w, double *__restrict__ d, u64 *__restrict__ ctr) {
    __shared__ u64 s_min;
    __shared__ unsigned int s_below;
    if (threadIdx.x == 0) {
        s_min = ~0ull;
        s_below = 0;
    }
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) {
        double p[3], nh[3], ws = 0.0, ds = 0.0;
        const bool ok = pv_valid(xyz, nrm, s, p, nh);
        const double r = ok ? rho[s] : 0.0;
        if (ok) {
            const double inv = 1.0 / (64.0 * r); // (r > 0: the sample counts itself; r = 0 would give inf and the clamp)
            ws = inv < 1.0 ? inv : 1.0;
            const double v = depth_in ? depth_in[s] : val[s];
            ds = v > (double)PD_LMIN ? v : (double)PD_LMIN; // (NaN lands on PD_LMIN)
            ds = ds < (double)depth ? ds : (double)depth;
            u64 bits;
            __builtin_memcpy(&bits, &ds, 8);
            atomicMin(&s_min, bits);
            if (ds < (double)depth) atomicAdd(&s_below, 1u);
        }
        rho[s] = r;
        w[s] = ws;
        d[s] = ds;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_min != ~0ull) atomicMin(ctr, s_min);
        if (s_below) atomicAdd(ctr + 1, (u64)s_below);
    }
}

// ---- 4: the level splat on the levels 3..box.top (occ may be NULL) -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pd_splat(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, PdBox box,
                                                  const double *__restrict__ w, const double *__restrict__ d, u64 *__restrict__ V,
                                                  uint8_t *__restrict__ occ) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double p[3], nh[3];
    if (!pv_valid(xyz, nrm, s, p, nh)) return;
    const int depth = box.depth;
    if (occ) { // occ: f7's cell on the finest level, clamped to the grid
        int c[3];
        pv_occ_cell3(p, box.g, c);
        occ[DenseSpace{depth}.elem(c[0], c[1], c[2])] = 1;
    }
    const double ws = w[s];
    int lo;
    const double fr = pd_split(d[s], depth, &lo);
    for (int t = 0; t < 2; t++) {
        const int L = lo + t;
        if (L > box.top) break; // (top <= depth: the levels above the buffer's top are another unit's)
        const double alpha = pd_alpha(fr, ws, t);
        const double an[3] = {alpha * nh[0], alpha * nh[1], alpha * nh[2]};
        pv_splat8(DenseSpace{L}, p, pd_level_grid(box, L), an, V + pd_level_word(L), pd_level_nodes(L));
    }
}

// ---- 5: one level of the cascade, in place: the word that held V_L holds U_L afterwards (a thread reads and writes its own word only; the
// coarser level is another part of the buffer).  grid.y = the component --------------------------------------------------------------------
__device__ __forceinline__ double pd_coarse(const double *__restrict__ A, int nc, int i, int j, int k) {
    return (i < 0 || j < 0 || k < 0 || i >= nc || j >= nc || k >= nc) ? 0.0 : A[(size_t)i + (size_t)nc * ((size_t)j + (size_t)nc * k)];
}
__global__ __launch_bounds__(256) void k_pd_cascade(u64 *fine, const double *__restrict__ coarse, int shf, double scale) {
    const int nf = 1 << shf, nc = nf >> 1;
    const size_t n3 = (size_t)1 << (3 * shf);
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n3) return;
    u64 *word = fine + (size_t)blockIdx.y * n3 + t;
    double u = ((double)(long long)*word / PV_FIX) * scale;
    if (coarse) {
        const double *A = coarse + (size_t)blockIdx.y * (n3 >> 3);
        const int i = (int)(t & (nf - 1)), j = (int)((t >> shf) & (nf - 1)), k = (int)(t >> (2 * shf));
        const int ci[2] = {i >> 1, (i >> 1) + ((i & 1) ? 1 : -1)}, cj[2] = {j >> 1, (j >> 1) + ((j & 1) ? 1 : -1)}, ck[2] = {k >> 1, (k >> 1) + ((k & 1) ? 1 : -1)};
        u = u + pd_prolong_at([=](int x, int y, int z) { return pd_coarse(A, nc, x, y, z); }, ci, cj, ck);
    }
    __builtin_memcpy(word, &u, 8);
}

// ---- 7: w_s chi(p_s) ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pd_mul(double *__restrict__ x, const double *__restrict__ w, int64_t n) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) x[s] = w[s] * x[s];
}

} // namespace

int poisson_density_samples_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, const double grid[4], int kernel_depth, double samples_per_node,
                                   const double *d_depth_in, double *d_rho, double *d_w, double *d_d, double sample_stats[3], hipStream_t st) {
    sample_stats[0] = sample_stats[1] = sample_stats[2] = 0.0;
    DevMem M;
    u64 *ctr = M.get<u64>(2);
    double *val = M.get<double>((size_t)n), *part = M.get<double>(POISSON_SUM_PARTIALS), *scal = M.get<double>(1);
    if (!M.ok) return RSM_E_NOMEM;
    const u64 init[2] = {~0ull, 0ull};
    DEVCHK(hipMemcpyAsync(ctr, init, sizeof init, hipMemcpyHostToDevice, st));
    // the density at the samples' own positions: they are float xyz of stride 3, as a mesh's vertices are
    int s = density_at_points_device(M, d_xyz, d_nrm4, n, depth, grid, kernel_depth, samples_per_node, d_xyz, n, d_rho, val, st);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL(k_pd_sample, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, depth, d_depth_in, (const double *)val, d_rho, d_w, d_d, ctr);
    poisson_tree_sum(d_w, n, part, scal, st);
    u64 h[2] = {0, 0};
    double sum_w = 0.0;
    DEVCHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
    DEVCHK(hipMemcpyAsync(&sum_w, scal, sizeof sum_w, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    if (h[0] != ~0ull) memcpy(&sample_stats[0], &h[0], 8);
    sample_stats[1] = (double)h[1];
    sample_stats[2] = sum_w;
    return RSM_OK;
}

size_t poisson_density_level_words(int top) { return pd_level_word(top + 1); }

int poisson_density_levels_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, int top, const double grid[4], const double *d_w, const double *d_d,
                                  unsigned long long *d_V, uint8_t *d_occ, const double **d_U_top, hipStream_t st) {
    DEVCHK(hipMemsetAsync(d_V, 0, pd_level_word(top + 1) * sizeof(u64), st));
    if (d_occ) DEVCHK(hipMemsetAsync(d_occ, 0, pd_level_nodes(depth), st));
    const PdBox box{pv_grid(grid, depth), depth, top};
    hipLaunchKernelGGL(k_pd_splat, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, box, d_w, d_d, d_V, d_occ);
    for (int L = PD_LMIN; L <= top; L++) {
        const double *coarse = L > PD_LMIN ? (const double *)(d_V + pd_level_word(L - 1)) : nullptr;
        hipLaunchKernelGGL(k_pd_cascade, dim3(blocks_for(pd_level_nodes(L)).x, 3), dim3(256), 0, st, d_V + pd_level_word(L), coarse, L, ldexp(1.0, 3 * (L - depth)));
    }
    *d_U_top = (const double *)(d_V + pd_level_word(top));
    return RSM_OK;
}

void poisson_density_rhs_of_field(const double *d_U, int depth, float *d_b32, double *d_b64, hipStream_t st) {
    hipLaunchKernelGGL((k_pv_rhs<DenseSpace, double>), blocks_for(pd_level_nodes(depth)), dim3(256), 0, st, d_U, DenseSpace{depth}, d_b32, d_b64);
}

int poisson_density_rhs_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, const double grid[4], int kernel_depth, double samples_per_node,
                               const double *d_depth_in, float *d_b32, double *d_b64, uint8_t *d_occ, double *d_rho, double *d_w, double *d_d,
                               double sample_stats[3], hipStream_t st) {
    sample_stats[0] = sample_stats[1] = sample_stats[2] = 0.0;
    DevMem M; // (all of the call's level buffer before its first launch)
    u64 *V = M.get<u64>(pd_level_word(depth + 1));
    if (!M.ok) return RSM_E_NOMEM;
    int s = poisson_density_samples_device(d_xyz, d_nrm4, n, depth, grid, kernel_depth, samples_per_node, d_depth_in, d_rho, d_w, d_d, sample_stats, st);
    if (s != RSM_OK) return s;
    const double *U = nullptr;
    if ((s = poisson_density_levels_device(d_xyz, d_nrm4, n, depth, depth, grid, d_w, d_d, V, d_occ, &U, st)) != RSM_OK) return s;
    poisson_density_rhs_of_field(U, depth, d_b32, d_b64, st);
    return mesh_finish(st);
}

int poisson_weighted_mean_device(double *d_val, const double *d_w, int64_t n, double sum_w, double *mean, hipStream_t st) {
    DevMem M;
    double *part = M.get<double>(POISSON_SUM_PARTIALS), *scal = M.get<double>(1);
    if (!M.ok) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_pd_mul, blocks_for((size_t)n), dim3(256), 0, st, d_val, d_w, n);
    poisson_tree_sum(d_val, n, part, scal, st);
    double sum = 0.0;
    DEVCHK(hipMemcpyAsync(&sum, scal, sizeof sum, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    *mean = sum / sum_w;
    return RSM_OK;
}

int poisson_iso_weighted_device(const float *d_xyz, const float *d_nrm4, int64_t n, const double *d_w, double sum_w, const float *d_chi, int depth,
                                const double grid[4], double *iso, hipStream_t st) {
    auto chi_at = [&](double *val) { poisson_chi_at_samples(d_xyz, d_nrm4, n, d_chi, depth, grid, val, st); };
    return poisson_mean_of_chi_at_samples(chi_at, n, d_w, sum_w, iso, st);
}
