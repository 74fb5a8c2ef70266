// k_poisson_band_density.hip -- the banded finest level (k_poisson_band.hip) with the density-adaptive splat
// (k_poisson_density.hip; f14): script1.mlx's OctDepth 10 and SamplesPerNode 3 together.  Restated in numpy in
// tests/poisson_band_density_restatement.py.  D = the finest depth; both halves state their rules once and are called here; what is new is
// the part in between:
//   levels 3..D-1   f14's level splat and cascade into a dense buffer whose top level is D - 1, with the scales 8^(L - D) -> W, fp64, three
//                   components on 2^(D-1) nodes per axis                                              poisson_density_levels_device
//   level D         a sample with d_s > D - 1 puts alpha = fr w_s (d_s = D: w_s) at its eight level-D nodes: f14's fixed-point terms
//                   llrint((wt (alpha n^_a)) 2^32) into brick-major V_D[3][S 512] through the slot table; 64-bit integer atomics.  With
//                   band_bricks >= 1 every such node is active; nodes outside the grid are dropped.  occ is f16's      k_pbd_splat
//   right-hand side U_D(node) = V_D(node) 2^-32 + P(W)(node); P = f14's prolongation at one node (poisson_space.h's pd_prolong_at, which
//                   k_pd_cascade evaluates too; 0 outside the coarse grid); V_D = 0 at an inactive node, U_D = 0
//                   outside the fine grid.  b_f = 0.5 ((dx U_x + dy U_y) + dz U_z) in fp64 on every active node, rounded once to float for the
//                   band solver.  One workgroup per brick: the 6^3 coarse nodes under the brick and its halo of one fine node go to LDS per
//                   component, then each component's slab of U (10 x 8 x 8 along its own axis), then the differences.  The bits depend on
//                   the expressions only, not on this staging                                                            k_pbd_rhs
//   iso             sum w_s chi(p_s) / sum w_s: f16's chi at the samples, f14's product and f7's tree
// No float atomics.  Built with -ffp-contract=off (csrc/Makefile): every fp64 expression below is evaluated as written.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"
#include "poisson_space.h"
#include "poisson_density_common.h"

#include <math.h>

namespace {

typedef unsigned long long u64;

// ---- level D of the splat, on the bricks ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pbd_splat(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, MtGrid g, BandSpace S,
                                                   const double *__restrict__ w, const double *__restrict__ d, u64 *__restrict__ V /* [3][S 512] */,
                                                   uint8_t *__restrict__ occ) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double p[3], nh[3];
    if (!pv_valid(xyz, nrm, s, p, nh)) return;
    int c[3];
    pv_occ_cell3(p, g, c); // occ: f16's cell, clamped to the grid
    const long long ce = S.elem(c[0], c[1], c[2]);
    if (ce >= 0) occ[ce] = 1; // (the cell's brick is occupied, so active)
    int lo;
    const double fr = pd_split(d[s], S.B.sh, &lo);
    const int t = S.B.sh - lo; // level D is lo (t = 0) or lo + 1 (t = 1)
    if (t > 1) return;
    const double alpha = pd_alpha(fr, w[s], t);
    const double an[3] = {alpha * nh[0], alpha * nh[1], alpha * nh[2]};
    pv_splat8(S, p, g, an, V, S.nodes());
}

// ---- the right-hand side: one workgroup of 256 threads per brick --------------------------------------------------------------------------
#define PBD_CW 6                          // coarse nodes per axis under a brick and its halo: fine -1..8 -> coarse (o >> 1) - 1 .. (o >> 1) + 4
#define PBD_CN (PBD_CW * PBD_CW * PBD_CW) // 216
#define PBD_SLAB 640                      // a component's U: 10 along its own axis (fine -1..8), 8 x 8 across
// per axis, for the fine local coordinate l in -1..8 (the brick's origin is even): the near and the far coarse node, as places in the 6-wide block
__device__ __forceinline__ void pbd_near_far(int l, int &nr, int &fa) {
    nr = (l >> 1) + 1;
    fa = nr + ((l & 1) ? 1 : -1);
}
__global__ __launch_bounds__(256) void k_pbd_rhs(const long long *__restrict__ V, size_t nodes, PbBand B, const double *__restrict__ W /* [3][(N/2)^3] */,
                                                 float *__restrict__ b32, double *__restrict__ b64) {
    __shared__ double sW[3][PBD_CN];
    __shared__ double sU[3][PBD_SLAB];
    __shared__ int32_t nb[27];
    const int slot = blockIdx.x;
    if (threadIdx.x < 27) nb[threadIdx.x] = B.nbr[(size_t)slot * 27 + threadIdx.x];
    int o[3];
    pb_origin(B, slot, o);
    const int nc = B.N >> 1;
    const size_t nc3 = (size_t)nc * nc * nc;
    for (int t = threadIdx.x; t < 3 * PBD_CN; t += 256) { // W under the brick, 0 outside the coarse grid
        const int a = t / PBD_CN, r = t % PBD_CN;
        const int x = (o[0] >> 1) - 1 + r % PBD_CW, y = (o[1] >> 1) - 1 + (r / PBD_CW) % PBD_CW, z = (o[2] >> 1) - 1 + r / (PBD_CW * PBD_CW);
        sW[a][r] = (x < 0 || y < 0 || z < 0 || x >= nc || y >= nc || z >= nc) ? 0.0 : W[a * nc3 + (size_t)x + (size_t)nc * ((size_t)y + (size_t)nc * z)];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 3 * PBD_SLAB; t += 256) { // U_a = V_a 2^-32 + P(W_a) where component a's differences read it
        const int a = t / PBD_SLAB, r = t % PBD_SLAB;
        const int u = r % 10 - 1, v = (r / 10) & 7, q = r / 80;
        const int l[3] = {a == 0 ? u : v, a == 0 ? v : (a == 1 ? u : q), a == 2 ? u : q}; // (selects: no dynamic index, it stays in registers)
        const long long e = pb_node(nb, l[0], l[1], l[2]);
        double U = 0.0; // outside the fine grid
        if (e != -2) {
            const double own = e >= 0 ? (double)V[a * nodes + (size_t)e] / PV_FIX : 0.0; // (k_pd_cascade's scale is 8^0 here)
            const double *A = sW[a];
            int ci[2], cj[2], ck[2];
            pbd_near_far(l[0], ci[0], ci[1]);
            pbd_near_far(l[1], cj[0], cj[1]);
            pbd_near_far(l[2], ck[0], ck[1]);
            U = own + pd_prolong_at([=](int x, int y, int z) { return A[x + PBD_CW * (y + PBD_CW * z)]; }, ci, cj, ck);
        }
        sU[a][r] = U;
    }
    __syncthreads();
    for (int h = 0; h < 2; h++) {
        const int n = threadIdx.x + 256 * h, x = n & 7, y = (n >> 3) & 7, z = n >> 6;
        const double dx = sU[0][(x + 2) + 10 * (y + 8 * z)] - sU[0][x + 10 * (y + 8 * z)];
        const double dy = sU[1][(y + 2) + 10 * (x + 8 * z)] - sU[1][y + 10 * (x + 8 * z)];
        const double dz = sU[2][(z + 2) + 10 * (x + 8 * y)] - sU[2][z + 10 * (x + 8 * y)];
        const double b = 0.5 * ((dx + dy) + dz);
        const size_t e = (size_t)slot * PB_NODES + n;
        if (b32) b32[e] = (float)b;
        if (b64) b64[e] = b;
    }
}

} // namespace

int poisson_band_density_rhs_device(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, const double grid[4], const double *d_w,
                                    const double *d_d, unsigned long long *d_levels, float *d_b32, double *d_b64, uint8_t *d_occ, hipStream_t st) {
    const size_t nodes = pb_nodes(band);
    if (nodes == 0) return RSM_OK;
    DevMem M; // (the call's scratch before its first launch)
    u64 *V = M.get<u64>(3 * nodes);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(V, 0, 3 * nodes * sizeof(u64), st));
    DEVCHK(hipMemsetAsync(d_occ, 0, nodes, st));
    const double *W = nullptr;
    const int s = poisson_density_levels_device(d_xyz, d_nrm4, n, band.depth, band.depth - 1, grid, d_w, d_d, d_levels, nullptr, &W, st);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL(k_pbd_splat, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, pv_grid(grid, band.depth), pb_space(band), d_w, d_d, V, d_occ);
    hipLaunchKernelGGL(k_pbd_rhs, dim3((unsigned)band.n_active), dim3(256), 0, st, (const long long *)V, nodes, pb_band(band), W, d_b32, d_b64);
    return mesh_finish(st);
}

int poisson_band_iso_weighted_device(const PoissonBand &band, const float *d_xyz, const float *d_nrm4, int64_t n, const double *d_w, double sum_w, const float *d_chi,
                                     const double grid[4], double *iso, hipStream_t st) {
    auto chi_at = [&](double *val) { poisson_band_chi_at_samples(band, d_xyz, d_nrm4, n, d_chi, grid, val, st); };
    return poisson_mean_of_chi_at_samples(chi_at, n, d_w, sum_w, iso, st);
}
