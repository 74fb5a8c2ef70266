// k_poisson.hip -- a surface from the smoothed, oriented cloud: where CCloudOptimization::run hands bigcloud.ply to
// meshlab.bat ("Surface Reconstruction: Poisson") and filter() hands a pair's cloud to mesh.bat (PoissonRecon --pointWeight 0, then
// SurfaceTrimmer), this file runs the published method (Kazhdan, Bolitho, Hoppe: Poisson Surface Reconstruction, SGP 2006) in its plain,
// unscreened form on a DENSE grid of N = 2^depth nodes per axis.  Not a bit-parity port of those tools (no source in the reference tree);
// the eight steps are defined in DESIGN.md 9 (f7) and restated in numpy in tests/poisson_restatement.py:
//   1 valid samples (finite point and normal, normal != 0, normalised in fp64)       k_pv_bbox
//   2 grid: o, h from the fp64 bounding box (host)
//   3 splat V = sum w n^ (trilinear, 8 nodes) into 64-bit fixed point, occ(cell)     k_pv_splat (pv_splat8)
//   4 b = 1/2 central differences of V (V = 0 outside)                               k_pv_rhs<DenseSpace, long long>
//   5 L chi = b, 7-point Laplacian, chi = 0 outside: conjugate gradients preconditioned by one cell-centred multigrid V-cycle
//     (red-black Gauss-Seidel, 8-cell mean restriction, piecewise-constant prolongation, rediscretised coarse operators down to 2^3)
//   6 iso = mean of chi at the samples (fp64, fixed summation tree)                  k_pv_chi_at_samples<DenseSpace> + k_pv_sum
//   7 marching tetrahedra on the node lattice (six Kuhn tetrahedra per cell), indexed by lattice edge: flag -> scan -> emit
//   8 trim by the dilated occupancy, compaction of faces and vertices
// Reproducibility: the splat adds llrint(w n^ 2^32) with 64-bit integer atomics -- integer sums do not depend on arrival order.  |w n^| <= 1
// and a sample meets a node at most once, so INT32_MAX samples sum to at most (2^31 - 1) 2^32 < 2^63.  Every floating-point reduction
// (dot products, the iso-value) runs over a grid that depends on the problem size only, block trees in LDS, then one block over the partials.
// Steps 3, 4, 6 and 7 are the rules DESIGN.md 9 f42 states once for this grid, the density-adaptive splat and the band of bricks
// (poisson_space.h, poisson_common.h), here on the DenseSpace; what is this file's own is the box, the multigrid solver and the summation tree.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"
#include "poisson_common.h"

#include <string.h>

#include <math.h>

#include <vector>

#define PV_RED_BLOCKS POISSON_SUM_PARTIALS // partial sums of a reduction (fixed: the summation tree depends on the size only)

namespace {

// ---- 1: valid samples and their bounding box: mm[0..2] = min, mm[3..5] = max (ordered uints), cnt[0] = valid ------------------
template <bool HAS_N>
__device__ __forceinline__ void pv_bbox_body(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, unsigned int *__restrict__ mm,
                                             unsigned long long *__restrict__ cnt) {
    __shared__ unsigned int s_mm[6];
    __shared__ unsigned int s_cnt;
    if (threadIdx.x < 6) s_mm[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += (int64_t)gridDim.x * blockDim.x) {
        double p[3], nh[3];
        if (!(HAS_N ? pv_valid(xyz, nrm, s, p, nh) : pv_valid_point(xyz, s, p))) continue;
        for (int a = 0; a < 3; a++) {
            const unsigned int o = f2ord(xyz[3 * s + a]);
            atomicMin(&s_mm[a], o);
            atomicMax(&s_mm[3 + a], o);
        }
        atomicAdd(&s_cnt, 1u);
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&mm[threadIdx.x], s_mm[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&mm[threadIdx.x], s_mm[threadIdx.x]);
    if (threadIdx.x == 0 && s_cnt) atomicAdd(cnt, (unsigned long long)s_cnt);
}
__global__ __launch_bounds__(256) void k_pv_bbox(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, unsigned int *__restrict__ mm,
                                                 unsigned long long *__restrict__ cnt) {
    pv_bbox_body<true>(xyz, nrm, n, mm, cnt);
}
// the density trim's samples without normals: a finite point is a valid sample
__global__ __launch_bounds__(256) void k_pv_bbox_points(const float *__restrict__ xyz, int64_t n, unsigned int *__restrict__ mm, unsigned long long *__restrict__ cnt) {
    pv_bbox_body<false>(xyz, nullptr, n, mm, cnt);
}

// ---- 3: splat (step 4, the right-hand side, is poisson_space.h's k_pv_rhs) ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pv_splat(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, MtGrid g, DenseSpace S,
                                                  unsigned long long *__restrict__ V /* [3][N^3] */, uint8_t *__restrict__ occ) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double p[3], nh[3];
    if (!pv_valid(xyz, nrm, s, p, nh)) return;
    int c[3];
    pv_occ_cell3(p, g, c);
    occ[S.elem(c[0], c[1], c[2])] = 1;
    pv_splat8(S, p, g, nh, V, S.nodes());
}

// ---- reductions ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void block_sum_to(double v, double *dst) { // 256 threads, fixed tree
    __shared__ double s[256];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dst = s[0];
}
__global__ __launch_bounds__(256) void k_pv_sum(const double *__restrict__ part, int m, double *__restrict__ out) { // one block
    double a = 0.0;
    for (int t = threadIdx.x; t < m; t += 256) a += part[t];
    block_sum_to(a, out);
}
__global__ __launch_bounds__(256) void k_pv_sum_f64(const double *__restrict__ v, int64_t n, double *__restrict__ part) {
    double a = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) a += v[t];
    block_sum_to(a, &part[blockIdx.x]);
}
__global__ __launch_bounds__(256) void k_pv_dot(const float *__restrict__ x, const float *__restrict__ y, size_t n, double *__restrict__ part) {
    double a = 0.0;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (size_t)gridDim.x * 256) a += (double)x[t] * (double)y[t];
    block_sum_to(a, &part[blockIdx.x]);
}

// ---- 5: the Laplacian and the multigrid pieces (level of n = 1 << sh nodes per axis, chi = 0 outside) ---------------------------------
__device__ __forceinline__ float pv_nbr_sum(const float *__restrict__ x, size_t idx, int i, int j, int k, int n) {
    const size_t sy = (size_t)n, sz = (size_t)n * n;
    const float xm = i > 0 ? x[idx - 1] : 0.0f, xp = i + 1 < n ? x[idx + 1] : 0.0f;
    const float ym = j > 0 ? x[idx - sy] : 0.0f, yp = j + 1 < n ? x[idx + sy] : 0.0f;
    const float zm = k > 0 ? x[idx - sz] : 0.0f, zp = k + 1 < n ? x[idx + sz] : 0.0f;
    return ((xm + xp) + (ym + yp)) + (zm + zp);
}
// MODE 0: out = L x, partial sums of x . out;  1: out = b - L x, partial sums of out^2;  2: out = b - L x
template <int MODE>
__global__ __launch_bounds__(256) void k_pv_stencil(const float *__restrict__ x, const float *__restrict__ b, float *__restrict__ out, int sh,
                                                    double *__restrict__ part) {
    const int n = 1 << sh;
    const size_t n3 = (size_t)1 << (3 * sh);
    double acc = 0.0;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < n3; idx += (size_t)gridDim.x * 256) {
        const int i = (int)(idx & (n - 1)), j = (int)((idx >> sh) & (n - 1)), k = (int)(idx >> (2 * sh));
        const float c = x[idx];
        const float lx = pv_nbr_sum(x, idx, i, j, k, n) - 6.0f * c;
        if (MODE == 0) {
            out[idx] = lx;
            acc += (double)c * (double)lx;
        } else {
            const float r = b[idx] - lx;
            out[idx] = r;
            if (MODE == 1) acc += (double)r * (double)r;
        }
    }
    if (MODE != 2) block_sum_to(acc, &part[blockIdx.x]);
}
// one colour of a red-black Gauss-Seidel sweep: x = (sum of neighbours - b) / 6 on the nodes with (i + j + k) & 1 == colour
__global__ __launch_bounds__(256) void k_pv_rbgs(float *__restrict__ x, const float *__restrict__ b, int sh, int colour) {
    const int n = 1 << sh;
    const size_t half = (size_t)1 << (3 * sh - 1);
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= half) return;
    const int ih = (int)(t & ((n >> 1) - 1)), j = (int)((t >> (sh - 1)) & (n - 1)), k = (int)(t >> (2 * sh - 1));
    const int i = 2 * ih + ((j + k + colour) & 1);
    const size_t idx = (size_t)i + (size_t)n * ((size_t)j + (size_t)n * k);
    x[idx] = (pv_nbr_sum(x, idx, i, j, k, n) - b[idx]) / 6.0f;
}
// coarse right-hand side: the coarse operator is the same stencil at spacing 2h, so b_c = 4 * mean of the 8 fine residuals
__global__ __launch_bounds__(256) void k_pv_restrict(const float *__restrict__ rf, float *__restrict__ bc, int shc) {
    const int nc = 1 << shc, nf = nc << 1;
    const size_t n3 = (size_t)1 << (3 * shc);
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n3) return;
    const int i = (int)(t & (nc - 1)), j = (int)((t >> shc) & (nc - 1)), k = (int)(t >> (2 * shc));
    const size_t f = (size_t)(2 * i) + (size_t)nf * ((size_t)(2 * j) + (size_t)nf * (2 * k));
    const size_t sy = (size_t)nf, sz = (size_t)nf * nf;
    const float s = (((rf[f] + rf[f + 1]) + (rf[f + sy] + rf[f + sy + 1])) + ((rf[f + sz] + rf[f + sz + 1]) + (rf[f + sz + sy] + rf[f + sz + sy + 1])));
    bc[t] = 0.5f * s;
}
__global__ __launch_bounds__(256) void k_pv_prolong_add(float *__restrict__ xf, const float *__restrict__ xc, int shf) {
    const int nf = 1 << shf;
    const size_t n3 = (size_t)1 << (3 * shf);
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n3) return;
    const int i = (int)(t & (nf - 1)), j = (int)((t >> shf) & (nf - 1)), k = (int)(t >> (2 * shf));
    const int nc = nf >> 1;
    xf[t] += xc[(size_t)(i >> 1) + (size_t)nc * ((size_t)(j >> 1) + (size_t)nc * (k >> 1))];
}
// ---- host ---------------------------------------------------------------------------------------------------------------------------
static inline unsigned red_blocks(size_t n) { return (unsigned)std::min<size_t>(PV_RED_BLOCKS, (n + 255) / 256); }

} // namespace

void poisson_mesh_free(PoissonMesh *m) {
    if (!m) return;
    if (m->d_v) (void)hipFree(m->d_v);
    if (m->d_f) (void)hipFree(m->d_f);
    m->d_v = nullptr;
    m->d_f = nullptr;
    m->nv = m->nf = 0;
}

int poisson_grid_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, double scale, double grid[4], int64_t counts[2],
                        hipStream_t st) {
    grid[0] = grid[1] = grid[2] = grid[3] = 0.0;
    counts[0] = 0;
    counts[1] = n;
    if (n <= 0) return RSM_OK;
    DevMem M;
    unsigned int *mm = M.get<unsigned int>(8);
    unsigned long long *cnt = M.get<unsigned long long>(1);
    if (!M.ok) return RSM_E_NOMEM;
    const unsigned int init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    DEVCHK(hipMemcpyAsync(mm, init, sizeof init, hipMemcpyHostToDevice, st));
    DEVCHK(hipMemsetAsync(cnt, 0, sizeof *cnt, st));
    if (d_nrm4) hipLaunchKernelGGL(k_pv_bbox, dim3(red_blocks((size_t)n)), dim3(256), 0, st, d_xyz, d_nrm4, n, mm, cnt);
    else hipLaunchKernelGGL(k_pv_bbox_points, dim3(red_blocks((size_t)n)), dim3(256), 0, st, d_xyz, n, mm, cnt);
    unsigned int h_mm[6];
    unsigned long long h_cnt = 0;
    DEVCHK(hipMemcpyAsync(h_mm, mm, sizeof h_mm, hipMemcpyDeviceToHost, st));
    DEVCHK(hipMemcpyAsync(&h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    counts[0] = (int64_t)h_cnt;
    counts[1] = n - (int64_t)h_cnt;
    if (h_cnt == 0) return RSM_OK;
    double lo[3], hi[3], ext = 0.0;
    for (int a = 0; a < 3; a++) {
        lo[a] = (double)ord2f(h_mm[a]);
        hi[a] = (double)ord2f(h_mm[3 + a]);
        ext = std::max(ext, hi[a] - lo[a]);
    }
    const double side = scale * ext;
    if (!(side > 0.0) || !std::isfinite(side)) return RSM_OK; // all points equal: h stays 0
    for (int a = 0; a < 3; a++) grid[a] = (lo[a] + hi[a]) / 2.0 - side / 2.0;
    grid[3] = side / (double)(1 << depth);
    return RSM_OK;
}

int poisson_rhs_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, const double grid[4], float *d_b32, double *d_b64,
                       uint8_t *d_occ, hipStream_t st) {
    const size_t N3 = (size_t)1 << (3 * depth);
    DevMem M;
    unsigned long long *V = M.get<unsigned long long>(3 * N3);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(V, 0, 3 * N3 * sizeof(unsigned long long), st));
    DEVCHK(hipMemsetAsync(d_occ, 0, N3, st));
    const DenseSpace S{depth};
    hipLaunchKernelGGL(k_pv_splat, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, pv_grid(grid, depth), S, V, d_occ);
    hipLaunchKernelGGL((k_pv_rhs<DenseSpace, long long>), blocks_for(N3), dim3(256), 0, st, (const long long *)V, S, d_b32, d_b64);
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    return RSM_OK;
}

namespace {
struct Solver {
    int depth = 0;
    hipStream_t st = nullptr;
    std::vector<float *> x, b, r; // per level; level 0: x = z, b = the CG residual
    double *part = nullptr, *scal = nullptr;
    // what poisson_pcg's Ops read: the elements, the blocks of a reduction, the right-hand side, z = x[0]
    size_t n = 0;
    unsigned rb = 0;
    const float *rhs = nullptr;
    float *z = nullptr;
    int vcycle(int l) {
        const int sh = depth - l;
        const size_t n3 = (size_t)1 << (3 * sh);
        const dim3 gh = blocks_for(n3 / 2);
        DEVCHK(hipMemsetAsync(x[l], 0, n3 * sizeof(float), st));
        if (sh == 1) { // 2^3: 8 red-black sweeps, then 8 black-red (symmetric)
            for (int s = 0; s < 16; s++)
                for (int c = 0; c < 2; c++) hipLaunchKernelGGL(k_pv_rbgs, gh, dim3(256), 0, st, x[l], b[l], sh, s < 8 ? c : 1 - c);
            return RSM_OK;
        }
        for (int c = 0; c < 2; c++) hipLaunchKernelGGL(k_pv_rbgs, gh, dim3(256), 0, st, x[l], b[l], sh, c);
        hipLaunchKernelGGL(k_pv_stencil<2>, dim3(std::min<size_t>(4096, (n3 + 255) / 256)), dim3(256), 0, st, x[l], b[l], r[l], sh, (double *)nullptr);
        hipLaunchKernelGGL(k_pv_restrict, blocks_for(n3 / 8), dim3(256), 0, st, r[l], b[l + 1], sh - 1);
        const int s = vcycle(l + 1);
        if (s != RSM_OK) return s;
        hipLaunchKernelGGL(k_pv_prolong_add, blocks_for(n3), dim3(256), 0, st, x[l], x[l + 1], sh);
        for (int c = 0; c < 2; c++) hipLaunchKernelGGL(k_pv_rbgs, gh, dim3(256), 0, st, x[l], b[l], sh, 1 - c);
        return RSM_OK;
    }
    int fetch(int m, double *out) { // the sum of `m` partials
        hipLaunchKernelGGL(k_pv_sum, dim3(1), dim3(256), 0, st, part, m, scal);
        DEVCHK(hipMemcpyAsync(out, scal, sizeof(double), hipMemcpyDeviceToHost, st));
        DEVCHK(hipStreamSynchronize(st));
        return RSM_OK;
    }
    // poisson_pcg's Ops: one V-cycle as the preconditioner; r = b[0], z = x[0]
    int precondition(double *rho) {
        const int s = vcycle(0);
        if (s != RSM_OK) return s;
        hipLaunchKernelGGL(k_pv_dot, dim3(rb), dim3(256), 0, st, (const float *)b[0], (const float *)z, n, part);
        return fetch((int)rb, rho);
    }
    int apply(const float *p, float *q, double *pq) {
        hipLaunchKernelGGL(k_pv_stencil<0>, dim3(rb), dim3(256), 0, st, p, (const float *)nullptr, q, depth, part);
        return fetch((int)rb, pq);
    }
    int residual(const float *chi, double *rr) {
        hipLaunchKernelGGL(k_pv_stencil<1>, dim3(rb), dim3(256), 0, st, chi, rhs, b[0], depth, part);
        return fetch((int)rb, rr);
    }
};
} // namespace

int poisson_solve_device(const float *d_b, int depth, double rel_residual, int max_cycles, float *d_chi, double *residual, int *cycles,
                         double *history, hipStream_t st) {
    const size_t N3 = (size_t)1 << (3 * depth);
    *residual = 0.0;
    *cycles = 0;
    DevMem M;
    Solver S;
    S.depth = depth;
    S.st = st;
    for (int l = 0; l < depth; l++) { // levels of 2^depth ... 2 nodes per axis
        const size_t n3 = (size_t)1 << (3 * (depth - l));
        S.x.push_back(M.get<float>(n3));
        S.b.push_back(M.get<float>(n3));
        S.r.push_back(M.get<float>(n3));
    }
    float *p = M.get<float>(N3), *q = M.get<float>(N3), *best = M.get<float>(N3);
    S.part = M.get<double>(PV_RED_BLOCKS);
    S.scal = M.get<double>(1);
    if (!M.ok) return RSM_E_NOMEM;
    S.n = N3;
    S.rhs = d_b;
    S.z = S.x[0];
    float *r = S.b[0];
    const unsigned rb = S.rb = red_blocks(N3);
    DEVCHK(hipMemsetAsync(d_chi, 0, N3 * sizeof(float), st));
    DEVCHK(hipMemcpyAsync(r, d_b, N3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    double bb = 0.0;
    hipLaunchKernelGGL(k_pv_dot, dim3(rb), dim3(256), 0, st, d_b, d_b, N3, S.part);
    int s = S.fetch((int)rb, &bb);
    if (s != RSM_OK) return s;
    if (!(bb > 0.0)) return RSM_OK; // b = 0: chi = 0
    DEVCHK(hipMemsetAsync(best, 0, N3 * sizeof(float), st)); // (chi = 0, residual 1)
    *residual = 1.0;
    if ((s = poisson_pcg(S, sqrt(bb), rel_residual, max_cycles, 2, d_chi, p, q, best, residual, cycles, history, st)) != RSM_OK) return s;
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    return *residual <= rel_residual ? RSM_OK : RSM_W_NOT_CONVERGED;
}

void poisson_chi_at_samples(const float *d_xyz, const float *d_nrm4, int64_t n, const float *d_chi, int depth, const double grid[4], double *d_val,
                            hipStream_t st) {
    hipLaunchKernelGGL(k_pv_chi_at_samples<DenseSpace>, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, pv_grid(grid, depth), DenseSpace{depth}, d_chi, d_val);
}

void poisson_tree_sum(const double *d_v, int64_t n, double *d_part, double *d_sum, hipStream_t st) {
    const unsigned rb = red_blocks((size_t)n);
    hipLaunchKernelGGL(k_pv_sum_f64, dim3(rb), dim3(256), 0, st, d_v, n, d_part);
    hipLaunchKernelGGL(k_pv_sum, dim3(1), dim3(256), 0, st, (const double *)d_part, (int)rb, d_sum);
}

int poisson_iso_device(const float *d_xyz, const float *d_nrm4, int64_t n, int64_t n_valid, const float *d_chi, int depth, const double grid[4],
                       double *iso, hipStream_t st) {
    auto chi_at = [&](double *val) { poisson_chi_at_samples(d_xyz, d_nrm4, n, d_chi, depth, grid, val, st); };
    return poisson_mean_of_chi_at_samples(chi_at, n, nullptr, (double)n_valid, iso, st);
}

// step 8's second half, for poisson_common.h's extraction: of `full` (its vertices flagged by vkeep) the faces whose
// three vertices are kept, the vertices they use, both renumbered in order -> *out; `full` is freed
int poisson_trim_commit(DevMem &M, PoissonMesh &full, const uint8_t *vkeep, PoissonMesh *out, hipStream_t st) {
    const uint64_t nv = (uint64_t)full.nv, nf = (uint64_t)full.nf;
    float *verts = full.d_v;
    int32_t *faces = full.d_f;
    int s;
    // trim: faces whose three vertices lie in the dilated occupancy, the vertices they use, both renumbered in order
    unsigned int *fkeep = M.get<unsigned int>(nf), *fpos = M.get<unsigned int>(nf), *vused = M.get<unsigned int>(nv), *vpos = M.get<unsigned int>(nv);
    s = M.ok ? RSM_OK : RSM_E_NOMEM;
    uint64_t kf = 0, kv = 0;
    if (s == RSM_OK && hipMemsetAsync(vused, 0, nv * sizeof(unsigned int), st) != hipSuccess) s = RSM_E_HIP;
    if (s == RSM_OK) {
        hipLaunchKernelGGL(k_pv_face_keep<>, blocks_for(nf), dim3(256), 0, st, (const int32_t *)faces, (size_t)nf, (const uint8_t *)vkeep, fkeep, vused);
        s = scan_u32(M, (const unsigned int *)fkeep, fpos, nf, st);
    }
    if (s == RSM_OK) s = scan_u32(M, (const unsigned int *)vused, vpos, nv, st);
    if (s == RSM_OK) s = scan_total(fkeep, fpos, nf, st, &kf);
    if (s == RSM_OK) s = scan_total(vused, vpos, nv, st, &kv);
    if (s == RSM_OK && kf > 0) {
        PoissonMesh kept;
        if ((s = mesh_result_alloc(kept, kv, kf)) == RSM_OK) {
            hipLaunchKernelGGL(k_mesh_compact_faces<>, blocks_for(nf), dim3(256), 0, st, (const int32_t *)faces, (size_t)nf, (const unsigned int *)fkeep,
                               (const unsigned int *)fpos, (const unsigned int *)vpos, kept.d_f);
            hipLaunchKernelGGL(k_mesh_compact_verts<>, blocks_for(nv), dim3(256), 0, st, (const float *)verts, (size_t)nv, (const unsigned int *)vused,
                               (const unsigned int *)vpos, kept.d_v);
            if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
                poisson_mesh_free(&kept);
                s = RSM_E_HIP;
            } else
                mesh_result_commit(out, kept);
        }
    }
    if (hipStreamSynchronize(st) != hipSuccess && s == RSM_OK) s = RSM_E_HIP;
    poisson_mesh_free(&full);
    return s;
}

int poisson_extract_device(const float *d_chi, int depth, double iso, const double grid[4], const uint8_t *d_occ, int trim_cells,
                           PoissonMesh *out, int64_t untrimmed[2], hipStream_t st) {
    const DenseSpace S{depth};
    auto dilate = [&](const uint8_t *in, uint8_t *to, int axis) {
        hipLaunchKernelGGL(k_pv_dilate<>, blocks_for(S.nodes()), dim3(256), 0, st, in, to, depth, axis, trim_cells);
    };
    return poisson_extract(S, pv_grid(grid, depth), d_chi, iso, d_occ, trim_cells, dilate, out, untrimmed, st);
}
