// k_meshstitch.hip -- levels the views' exposure seams in the mesh's colours: the other half of TextureStitcher's job at the end of
// CCloudOptimization::run (CCloudOptimization.cpp:394-397).  Not a port (no source in the reference tree): every rule is
// defined in DESIGN.md 9 (f10) and restated in numpy in tests/meshstitch_restatement.py, and the kernels are held to that restatement
// exactly.  Per channel, over the coloured vertices, the screened gradient-domain system
//     (A x)_i = sum over i's incidences of (x_i - x_j) + lambda x_i  =  G_i + lambda c_i,      G_i = sum of the target differences g_ij
// with c the best-view colouring (mode 0 of k_meshcolor.hip), g_ij = c_i - c_j inside a view and the views' own differences across a seam.
//   neighbour CSR   per coloured vertex its coloured neighbours in the order of its corner list (ascending 3 f + j, per corner
//                   f[(j+1)%3] then f[(j+2)%3]): an interior edge twice, a border edge once.  Row i starts at 2 row[i] (a corner gives at
//                   most two), deg[i] entries; dmax by an integer atomicMax                                                    k_mst_csr
//   right-hand side G and the five incidence counters; all g are multiples of 1/2 of magnitude <= 255: exact in fp64      k_mst_rhs
//   solver          Jacobi-preconditioned Chebyshev iteration, a fixed number of steps, coefficients from the host: no dot product, no
//                   reduction, no host synchronisation inside the loop; one launch per step, x ping-pong, d in place     k_mst_init, k_mst_step
//   residual        ||b - A x|| / ||b - A c||, once, after the loop: fixed-order two-stage sums                          k_mst_resid, k_mst_sum2
//   bytes           clamp(floor(x + 0.5), 0, 255), the largest |x - c| by an integer atomicMax on the double's bits      k_mst_finish
// No float atomics.  Built with -ffp-contract=off (csrc/Makefile): every expression below is evaluated as written.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "meshcolor_common.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace {

typedef unsigned long long u64;

// the counters: S_INC .. S_NONE are the stage's counts[5]
enum { S_INC = 0, S_SEAM, S_TWO, S_ONE, S_NONE, S_CLAMP, S_MAXDIFF, S_DMAX, S_N };
#define MST_RED_BLOCKS 256

__device__ __forceinline__ void add_if(u64 n, u64 *ctr) {
    if (n) atomicAdd(ctr, n);
}

// ---- the neighbour CSR ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mst_csr(const int32_t *__restrict__ best, size_t nv, const int32_t *__restrict__ f, const uint32_t *__restrict__ row,
                                                 const uint32_t *__restrict__ corner, uint32_t *__restrict__ nbr, uint32_t *__restrict__ deg, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    uint32_t n = 0;
    if (best[i] >= 0) {
        const size_t base = 2 * (size_t)row[i];
        for (uint32_t r = row[i]; r < row[i + 1]; r++) {
            const uint32_t c = corner[r];
            const size_t fi = c / 3;
            const uint32_t j = c % 3;
            const int32_t a = f[3 * fi + (j + 1) % 3], b = f[3 * fi + (j + 2) % 3];
            if (best[a] >= 0) nbr[base + n++] = (uint32_t)a;
            if (best[b] >= 0) nbr[base + n++] = (uint32_t)b;
        }
    }
    deg[i] = n;
    // (a stale read only costs an atomic that changes nothing)
    if ((u64)n > __hip_atomic_load(ctr + S_DMAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(ctr + S_DMAX, (u64)n);
}

// ---- the right-hand side --------------------------------------------------------------------------------------------------------------
// col_v(j): texture_color's pixel of vertex j in view v as red, green, blue; (127, 127, 127) where texture_color answers that
__device__ __forceinline__ void mst_col(const McView &c, const float *__restrict__ p, size_t j, double *r, double *g, double *b) {
    float q0, q1, q2;
    mcol_q(c, p[3 * j], p[3 * j + 1], p[3 * j + 2], &q0, &q1, &q2);
    size_t pix;
    *r = *g = *b = 127.0;
    if (mcol_pixel(q0, q1, q2, c.W, c.H, &pix)) {
        *b = (double)c.img[3 * pix];
        *g = (double)c.img[3 * pix + 1];
        *r = (double)c.img[3 * pix + 2];
    }
}

__global__ __launch_bounds__(256) void k_mst_rhs(const float *__restrict__ p, size_t nv, const int32_t *__restrict__ best, const uint8_t *__restrict__ rgb,
                                                 const u64 *__restrict__ vis, const McView *__restrict__ views, int seam_gradient, const uint32_t *__restrict__ row,
                                                 const uint32_t *__restrict__ deg, const uint32_t *__restrict__ nbr, double *__restrict__ G, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    double G0 = 0.0, G1 = 0.0, G2 = 0.0;
    u64 n_seam = 0, n_two = 0, n_one = 0, n_none = 0;
    const uint32_t n = deg[i];
    if (n) {
        const int a = best[i];
        const double ci0 = (double)rgb[3 * i], ci1 = (double)rgb[3 * i + 1], ci2 = (double)rgb[3 * i + 2];
        const size_t base = 2 * (size_t)row[i];
        for (uint32_t t = 0; t < n; t++) {
            const size_t j = nbr[base + t];
            const int b = best[j];
            const double cj0 = (double)rgb[3 * j], cj1 = (double)rgb[3 * j + 1], cj2 = (double)rgb[3 * j + 2];
            double g0, g1, g2;
            if (a == b) {
                g0 = ci0 - cj0;
                g1 = ci1 - cj1;
                g2 = ci2 - cj2;
            } else {
                n_seam++;
                g0 = g1 = g2 = 0.0;
                const bool a_sees_j = seam_gradient && ((vis[j] >> a) & 1), b_sees_i = seam_gradient && ((vis[i] >> b) & 1);
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
                if (a_sees_j) { // view a's own difference c_i - col_a(j)
                    double r_, g_, b_;
                    mst_col(views[a], p, j, &r_, &g_, &b_);
                    a0 = ci0 - r_;
                    a1 = ci1 - g_;
                    a2 = ci2 - b_;
                }
                if (b_sees_i) { // view b's own difference col_b(i) - c_j
                    double r_, g_, b_;
                    mst_col(views[b], p, i, &r_, &g_, &b_);
                    b0 = r_ - cj0;
                    b1 = g_ - cj1;
                    b2 = b_ - cj2;
                }
                if (a_sees_j && b_sees_i) {
                    n_two++;
                    g0 = (a0 + b0) / 2.0;
                    g1 = (a1 + b1) / 2.0;
                    g2 = (a2 + b2) / 2.0;
                } else if (a_sees_j) {
                    n_one++;
                    g0 = a0, g1 = a1, g2 = a2;
                } else if (b_sees_i) {
                    n_one++;
                    g0 = b0, g1 = b1, g2 = b2;
                } else
                    n_none++;
            }
            G0 = G0 + g0;
            G1 = G1 + g1;
            G2 = G2 + g2;
        }
    }
    G[3 * i] = G0;
    G[3 * i + 1] = G1;
    G[3 * i + 2] = G2;
    add_if((u64)n, ctr + S_INC);
    add_if(n_seam, ctr + S_SEAM);
    add_if(n_two, ctr + S_TWO);
    add_if(n_one, ctr + S_ONE);
    add_if(n_none, ctr + S_NONE);
}

// ---- the solver -----------------------------------------------------------------------------------------------------------------------
// x0 = c, d = 0, b = G + lambda c.  An uncoloured vertex gets b = lambda c whatever G holds: its residual is 0 and it stays c.
__global__ __launch_bounds__(256) void k_mst_init(size_t nv, const int32_t *__restrict__ best, const uint8_t *__restrict__ rgb, const double *__restrict__ G,
                                                  double lambda, double *__restrict__ x, double *__restrict__ d, double *__restrict__ b) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * nv) return;
    const double c = (double)rgb[t];
    x[t] = c;
    d[t] = 0.0;
    b[t] = (best[t / 3] >= 0 ? G[t] : 0.0) + lambda * c;
}

// S_i = sum over i's incidences of (x_i - x_j), in the CSR's order, for the three channels
__device__ __forceinline__ void mst_S(const double *__restrict__ x, const uint32_t *__restrict__ nbr, size_t base, uint32_t n, double x0, double x1, double x2,
                                      double *S0, double *S1, double *S2) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (uint32_t t = 0; t < n; t++) {
        const size_t j = nbr[base + t];
        s0 = s0 + (x0 - x[3 * j]);
        s1 = s1 + (x1 - x[3 * j + 1]);
        s2 = s2 + (x2 - x[3 * j + 2]);
    }
    *S0 = s0, *S1 = s1, *S2 = s2;
}

// one Chebyshev step, a thread per vertex: r = b - (S + lambda x), z = r / M, d = alpha d + beta z, x' = x + d
__global__ __launch_bounds__(256) void k_mst_step(size_t nv, const uint32_t *__restrict__ row, const uint32_t *__restrict__ deg, const uint32_t *__restrict__ nbr,
                                                  const double *__restrict__ x, const double *__restrict__ b, double *__restrict__ d, double *__restrict__ xo,
                                                  double lambda, double alpha, double beta) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const uint32_t n = deg[i];
    const double x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2];
    double S0, S1, S2;
    mst_S(x, nbr, 2 * (size_t)row[i], n, x0, x1, x2, &S0, &S1, &S2);
    const double M = (double)n + lambda;
    const double r0 = b[3 * i] - (S0 + lambda * x0), r1 = b[3 * i + 1] - (S1 + lambda * x1), r2 = b[3 * i + 2] - (S2 + lambda * x2);
    const double z0 = r0 / M, z1 = r1 / M, z2 = r2 / M;
    const double d0 = (alpha * d[3 * i]) + (beta * z0), d1 = (alpha * d[3 * i + 1]) + (beta * z1), d2 = (alpha * d[3 * i + 2]) + (beta * z2);
    d[3 * i] = d0;
    d[3 * i + 1] = d1;
    d[3 * i + 2] = d2;
    xo[3 * i] = x0 + d0;
    xo[3 * i + 1] = x1 + d1;
    xo[3 * i + 2] = x2 + d2;
}

// ---- the residual: fixed-order two-stage sums (the tree of k_poisson.hip's k_pv_dot / k_pv_sum) ------------------------------------------
__device__ __forceinline__ void mst_block_sum(double v, double *s, double *dst) { // 256 threads, fixed tree
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = s[0];
    __syncthreads();
}
// part[block] = sum of (b - A x)^2, part[gridDim.x + block] = sum of (b - A c)^2 over the block's vertices and the three channels
__global__ __launch_bounds__(256) void k_mst_resid(size_t nv, const uint32_t *__restrict__ row, const uint32_t *__restrict__ deg, const uint32_t *__restrict__ nbr,
                                                   const double *__restrict__ x, const double *__restrict__ c, const double *__restrict__ b, double lambda,
                                                   double *__restrict__ part) {
    __shared__ double s[256];
    double num = 0.0, den = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const uint32_t n = deg[i];
        const size_t base = 2 * (size_t)row[i];
        double S0, S1, S2;
        const double x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2];
        mst_S(x, nbr, base, n, x0, x1, x2, &S0, &S1, &S2);
        const double r0 = b[3 * i] - (S0 + lambda * x0), r1 = b[3 * i + 1] - (S1 + lambda * x1), r2 = b[3 * i + 2] - (S2 + lambda * x2);
        num += (r0 * r0 + r1 * r1) + r2 * r2;
        const double c0 = c[3 * i], c1 = c[3 * i + 1], c2 = c[3 * i + 2];
        mst_S(c, nbr, base, n, c0, c1, c2, &S0, &S1, &S2);
        const double q0 = b[3 * i] - (S0 + lambda * c0), q1 = b[3 * i + 1] - (S1 + lambda * c1), q2 = b[3 * i + 2] - (S2 + lambda * c2);
        den += (q0 * q0 + q1 * q1) + q2 * q2;
    }
    mst_block_sum(num, s, &part[blockIdx.x]);
    mst_block_sum(den, s, &part[gridDim.x + blockIdx.x]);
}
__global__ __launch_bounds__(256) void k_mst_sum2(const double *__restrict__ part, int m, double *__restrict__ out) { // one block
    __shared__ double s[256];
    for (int k = 0; k < 2; k++) {
        double a = 0.0;
        for (int t = threadIdx.x; t < m; t += 256) a += part[k * m + t];
        mst_block_sum(a, s, &out[k]);
    }
}
// c as doubles (the residual's denominator reads it through the same gather as x)
__global__ __launch_bounds__(256) void k_mst_bytes_f64(size_t n, const uint8_t *__restrict__ rgb, double *__restrict__ c) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) c[t] = (double)rgb[t];
}

// ---- the bytes ------------------------------------------------------------------------------------------------------------------------
// rgb holds c on entry and the levelled bytes on return (a thread reads and writes its own vertex only); uncoloured vertices stay
__global__ __launch_bounds__(256) void k_mst_finish(size_t nv, const int32_t *__restrict__ best, const double *__restrict__ x, uint8_t *rgb, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv || best[i] < 0) return;
    u64 clamped = 0;
    double big = 0.0;
    for (int k = 0; k < 3; k++) {
        const double v = x[3 * i + k], diff = fabs(v - (double)rgb[3 * i + k]);
        big = diff > big ? diff : big;
        double q = floor(v + 0.5);
        if (!(q >= 0.0 && q <= 255.0)) {
            clamped++;
            q = q > 255.0 ? 255.0 : 0.0;
        }
        rgb[3 * i + k] = (uint8_t)(int)q;
    }
    add_if(clamped, ctr + S_CLAMP);
    // (doubles >= 0 order as their bit patterns)
    const u64 bits = (u64)__double_as_longlong(big);
    if (bits > __hip_atomic_load(ctr + S_MAXDIFF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(ctr + S_MAXDIFF, bits);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
struct Csr {
    uint32_t *nbr = nullptr, *deg = nullptr;
    u64 *ctr = nullptr; // S_N counters, zeroed
};

// the neighbour CSR over the corner lists (row, corner: nv + 1 and 3 nf entries)
int build_csr(DevMem &M, const int32_t *d_best, size_t nv, const int32_t *d_f, size_t nf, const uint32_t *row, const uint32_t *corner, Csr *c, hipStream_t st) {
    c->nbr = M.get<uint32_t>(6 * nf);
    c->deg = M.get<uint32_t>(nv);
    c->ctr = M.get<u64>(S_N);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(c->ctr, 0, S_N * sizeof(u64), st));
    hipLaunchKernelGGL(k_mst_csr, blocks_for(nv), dim3(256), 0, st, d_best, nv, d_f, row, corner, c->nbr, c->deg, c->ctr);
    return RSM_OK;
}

// `steps` Chebyshev steps from x0 = c; *d_x = the buffer that holds the result; rel (may be NULL) = the relative residual after them
int solve(DevMem &M, size_t nv, const int32_t *d_best, const uint8_t *d_rgb, const double *d_G, const uint32_t *row, const Csr &c, u64 dmax, double lambda, int steps,
          double **d_x, double *rel, hipStream_t st) {
    double *xa = M.get<double>(3 * nv), *xb = M.get<double>(3 * nv), *d = M.get<double>(3 * nv), *b = M.get<double>(3 * nv);
    double *part = M.get<double>(2 * MST_RED_BLOCKS + 2);
    if (!M.ok) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_mst_init, blocks_for(3 * nv), dim3(256), 0, st, nv, d_best, d_rgb, d_G, lambda, xa, d, b);
    // the eigenvalues of M^-1 A lie in [lmin, 2]
    ChebSchedule cheb(lambda / ((double)dmax + lambda));
    for (int k = 0; k < steps; k++) {
        double alpha, beta;
        cheb.step(k, &alpha, &beta);
        hipLaunchKernelGGL(k_mst_step, blocks_for(nv), dim3(256), 0, st, nv, row, (const uint32_t *)c.deg, (const uint32_t *)c.nbr, (const double *)xa,
                           (const double *)b, d, xb, lambda, alpha, beta);
        double *t = xa;
        xa = xb;
        xb = t;
    }
    *d_x = xa;
    if (rel) {
        // (d is free after the last step: it takes c as doubles)
        hipLaunchKernelGGL(k_mst_bytes_f64, blocks_for(3 * nv), dim3(256), 0, st, 3 * nv, d_rgb, d);
        hipLaunchKernelGGL(k_mst_resid, dim3(MST_RED_BLOCKS), dim3(256), 0, st, nv, row, (const uint32_t *)c.deg, (const uint32_t *)c.nbr, (const double *)xa,
                           (const double *)d, (const double *)b, lambda, part);
        hipLaunchKernelGGL(k_mst_sum2, dim3(1), dim3(256), 0, st, (const double *)part, MST_RED_BLOCKS, part + 2 * MST_RED_BLOCKS);
        double h[2];
        DEVCHK(hipMemcpyAsync(h, part + 2 * MST_RED_BLOCKS, sizeof h, hipMemcpyDeviceToHost, st));
        DEVCHK(hipStreamSynchronize(st));
        DEVCHK(hipGetLastError());
        *rel = h[1] > 0.0 ? sqrt(h[0]) / sqrt(h[1]) : 0.0;
    }
    return RSM_OK;
}

} // namespace

int mesh_stitch_steps(double lambda, unsigned long long dmax, double reduction) {
    return cheb_steps(lambda / ((double)dmax + lambda), reduction, RSM_MESH_STITCH_MAX_ITERATIONS);
}

int mesh_visibility_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *p,
                           long long big_box, unsigned long long *d_vis, int *invalid, hipStream_t st) {
    DevMem M;
    McScene scene;
    uint8_t *rgb = M.get<uint8_t>(3 * (size_t)nv);
    if (!M.ok) return RSM_E_NOMEM;
    return mesh_color_scene_device(M, d_v, nv, d_f, nf, views, n_pairs, p, big_box, rgb, nullptr, d_vis, nullptr, invalid, &scene, st);
}

int mesh_stitch_rhs_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const rsm_dedup_view *views, int n_pairs, const uint8_t *d_rgb,
                           const int32_t *d_best, const unsigned long long *d_vis, int seam_gradient, double *d_G, int32_t *d_deg, int64_t counts[5], int *invalid,
                           hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    for (int k = 0; k < 5; k++) counts[k] = 0;
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK || nv == 0) return s;
    DevMem M;
    std::vector<McView> hv;
    McView *d_views = nullptr;
    if ((s = mesh_views_device(M, views, n_pairs, false, &hv, &d_views, invalid, st)) != RSM_OK) return s;
    uint32_t *row = nullptr, *corner = nullptr;
    if ((s = mesh_corner_lists(M, d_f, nv, nf, &row, &corner, st)) != RSM_OK) return s;
    Csr c;
    if ((s = build_csr(M, d_best, nv, d_f, nf, row, corner, &c, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_mst_rhs, blocks_for(nv), dim3(256), 0, st, d_v, nv, d_best, d_rgb, (const u64 *)d_vis, (const McView *)d_views, seam_gradient,
                       (const uint32_t *)row, (const uint32_t *)c.deg, (const uint32_t *)c.nbr, d_G, c.ctr);
    u64 h[S_N];
    DEVCHK(hipMemcpyAsync(h, c.ctr, sizeof h, hipMemcpyDeviceToHost, st));
    DEVCHK(hipMemcpyAsync(d_deg, c.deg, sizeof(uint32_t) * nv, hipMemcpyDeviceToDevice, st));
    DEVCHK(hipStreamSynchronize(st)); // (the views' host images were read by the copies above before this returns)
    DEVCHK(hipGetLastError());
    for (int k = 0; k < 5; k++) counts[k] = (int64_t)h[S_INC + k];
    return RSM_OK;
}

int mesh_stitch_solve_device(const int32_t *d_f, int64_t nv_, int64_t nf_, const int32_t *d_best, const uint8_t *d_rgb, const double *d_G, double lambda,
                             int iterations, double *d_x, double *rel_residual, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    *rel_residual = 0.0;
    int s = mesh_validate_device(nullptr, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK || nv == 0) return s;
    DevMem M;
    uint32_t *row = nullptr, *corner = nullptr;
    if ((s = mesh_corner_lists(M, d_f, nv, nf, &row, &corner, st)) != RSM_OK) return s;
    Csr c;
    if ((s = build_csr(M, d_best, nv, d_f, nf, row, corner, &c, st)) != RSM_OK) return s;
    u64 h[S_N];
    DEVCHK(hipMemcpyAsync(h, c.ctr, sizeof h, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    double *x = nullptr;
    if ((s = solve(M, nv, d_best, d_rgb, d_G, row, c, h[S_DMAX], lambda, iterations, &x, rel_residual, st)) != RSM_OK) return s;
    DEVCHK(hipMemcpyAsync(d_x, x, sizeof(double) * 3 * nv, hipMemcpyDeviceToDevice, st));
    DEVCHK(hipStreamSynchronize(st));
    return RSM_OK;
}

int mesh_stitch_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *cp,
                       const rsm_mesh_stitch_params *sp, long long big_box, uint8_t *d_rgb, int32_t *d_best, double *stats, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    double S[RSM_MESH_STITCH_STATS] = {0};
    S[0] = (double)nv;
    DevMem M;
    McScene scene;
    u64 *vis = M.get<u64>(nv);
    if (!d_best) d_best = M.get<int32_t>(nv);
    if (!M.ok) return RSM_E_NOMEM;
    double cs[RSM_MESH_COLOR_STATS];
    int s = mesh_color_scene_device(M, d_v, nv_, d_f, nf_, views, n_pairs, cp, big_box, d_rgb, d_best, vis, cs, invalid, &scene, st);
    if (s != RSM_OK) return s;
    S[1] = nv ? cs[1] : 0.0;
    if (S[1] > 0.0) {
        Csr c;
        if ((s = build_csr(M, d_best, nv, d_f, nf, scene.row, scene.corner, &c, st)) != RSM_OK) return s;
        double *G = M.get<double>(3 * nv);
        if (!M.ok) return RSM_E_NOMEM;
        hipLaunchKernelGGL(k_mst_rhs, blocks_for(nv), dim3(256), 0, st, d_v, nv, (const int32_t *)d_best, (const uint8_t *)d_rgb, (const u64 *)vis, scene.d_views,
                           sp->seam_gradient, scene.row, (const uint32_t *)c.deg, (const uint32_t *)c.nbr, G, c.ctr);
        u64 h[S_N];
        DEVCHK(hipMemcpyAsync(h, c.ctr, sizeof h, hipMemcpyDeviceToHost, st));
        DEVCHK(hipStreamSynchronize(st));
        DEVCHK(hipGetLastError());
        int steps = sp->iterations;
        if (steps == 0 && (steps = mesh_stitch_steps(sp->lambda, h[S_DMAX], sp->reduction)) < 0) {
            *invalid = 4;
            return RSM_E_INVALID;
        }
        double *x = nullptr, rel = 0.0;
        if ((s = solve(M, nv, d_best, d_rgb, G, scene.row, c, h[S_DMAX], sp->lambda, steps, &x, &rel, st)) != RSM_OK) return s;
        hipLaunchKernelGGL(k_mst_finish, blocks_for(nv), dim3(256), 0, st, nv, (const int32_t *)d_best, (const double *)x, d_rgb, c.ctr);
        DEVCHK(hipMemcpyAsync(h, c.ctr, sizeof h, hipMemcpyDeviceToHost, st));
        DEVCHK(hipStreamSynchronize(st));
        DEVCHK(hipGetLastError());
        for (int k = 0; k < 5; k++) S[2 + k] = (double)h[S_INC + k];
        S[7] = (double)h[S_DMAX];
        S[8] = (double)steps;
        S[9] = rel;
        S[10] = __builtin_bit_cast(double, h[S_MAXDIFF]);
        S[11] = (double)h[S_CLAMP];
    }
    if (stats) memcpy(stats, S, sizeof S);
    return RSM_OK;
}
