// k_poisson.hip -- a surface from the smoothed, oriented cloud: where CCloudOptimization::run hands bigcloud.ply to
// meshlab.bat ("Surface Reconstruction: Poisson") and filter() hands a pair's cloud to mesh.bat (PoissonRecon --pointWeight 0, then
// SurfaceTrimmer), this file runs the published method (Kazhdan, Bolitho, Hoppe: Poisson Surface Reconstruction, SGP 2006) in its plain,
// unscreened form on a DENSE grid of N = 2^depth nodes per axis.  Not a bit-parity port of those tools (no source in the reference tree);
// the eight steps are defined in DESIGN.md 9 (f7) and restated in numpy in tests/poisson_restatement.py:
//   1 valid samples (finite point and normal, normal != 0, normalised in fp64)       k_pv_bbox
//   2 grid: o, h from the fp64 bounding box (host)
//   3 splat V = sum w n^ (trilinear, 8 nodes) into 64-bit fixed point, occ(cell)     k_pv_splat
//   4 b = 1/2 central differences of V (V = 0 outside)                               k_pv_rhs
//   5 L chi = b, 7-point Laplacian, chi = 0 outside: conjugate gradients preconditioned by one cell-centred multigrid V-cycle
//     (red-black Gauss-Seidel, 8-cell mean restriction, piecewise-constant prolongation, rediscretised coarse operators down to 2^3)
//   6 iso = mean of chi at the samples (fp64, fixed summation tree)                  k_pv_iso + k_pv_sum
//   7 marching tetrahedra on the node lattice (six Kuhn tetrahedra per cell), indexed by lattice edge: flag -> scan -> emit
//   8 trim by the dilated occupancy, compaction of faces and vertices
// Reproducibility: the splat adds llrint(w n^ 2^32) with 64-bit integer atomics -- integer sums do not depend on arrival order.  |w n^| <= 1
// and a sample meets a node at most once, so INT32_MAX samples sum to at most (2^31 - 1) 2^32 < 2^63.  Every floating-point reduction
// (dot products, the iso-value) runs over a grid that depends on the problem size only, block trees in LDS, then one block over the partials.
// The density-adaptive form of steps 3, 4 and 6 (PoissonRecon's --samplesPerNode) is k_poisson_density.hip; it calls this
// file's solver, extraction, chi at the samples (poisson_chi_at_samples) and summation tree (poisson_tree_sum).
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

// ---- 3: splat -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pv_splat(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, PvGrid g,
                                                  unsigned long long *__restrict__ V /* [3][N^3] */, uint8_t *__restrict__ occ) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double p[3], nh[3];
    if (!pv_valid(xyz, nrm, s, p, nh)) return;
    const double o[3] = {g.ox, g.oy, g.oz};
    const int N = g.N;
    const size_t N3 = (size_t)N * N * N;
    int i0[3], c[3];
    double f[3];
    for (int a = 0; a < 3; a++) {
        const double u = (p[a] - o[a]) / g.h;
        const double gq = u - 0.5;
        const double fl = floor(gq);
        i0[a] = (int)fl;
        f[a] = gq - fl;
        int cc = (int)floor(u);
        c[a] = cc < 0 ? 0 : (cc > N - 1 ? N - 1 : cc);
    }
    occ[(size_t)c[0] + (size_t)N * ((size_t)c[1] + (size_t)N * c[2])] = 1;
    for (int dz = 0; dz < 2; dz++)
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const int i = i0[0] + dx, j = i0[1] + dy, k = i0[2] + dz;
                if (i < 0 || j < 0 || k < 0 || i >= N || j >= N || k >= N) continue;
                const double w = ((dx ? f[0] : 1.0 - f[0]) * (dy ? f[1] : 1.0 - f[1])) * (dz ? f[2] : 1.0 - f[2]);
                const size_t node = (size_t)i + (size_t)N * ((size_t)j + (size_t)N * k);
                for (int a = 0; a < 3; a++) {
                    const long long q = __double2ll_rn((w * nh[a]) * PV_FIX);
                    if (q) atomicAdd(&V[a * N3 + node], (unsigned long long)q);
                }
            }
}

// ---- 4: right-hand side (exact in integers, then one conversion) ------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pv_rhs(const long long *__restrict__ V, int sh, float *__restrict__ b32, double *__restrict__ b64) {
    const int N = 1 << sh;
    const size_t N3 = (size_t)1 << (3 * sh);
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N3) return;
    const int i = (int)(idx & (N - 1)), j = (int)((idx >> sh) & (N - 1)), k = (int)(idx >> (2 * sh));
    const size_t sy = (size_t)N, sz = (size_t)N * N;
    const long long *Vx = V, *Vy = V + N3, *Vz = V + 2 * N3;
    const long long dx = (i + 1 < N ? Vx[idx + 1] : 0) - (i > 0 ? Vx[idx - 1] : 0);
    const long long dy = (j + 1 < N ? Vy[idx + sy] : 0) - (j > 0 ? Vy[idx - sy] : 0);
    const long long dz = (k + 1 < N ? Vz[idx + sz] : 0) - (k > 0 ? Vz[idx - sz] : 0);
    const double b = (0.5 * (((double)dx + (double)dy) + (double)dz)) / PV_FIX;
    if (b32) b32[idx] = (float)b;
    if (b64) b64[idx] = b;
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
__global__ __launch_bounds__(256) void k_pv_axpy(float *__restrict__ y, const float *__restrict__ x, float a, size_t n) { // y += a x
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) y[t] = y[t] + a * x[t];
}
__global__ __launch_bounds__(256) void k_pv_xpay(float *__restrict__ y, const float *__restrict__ x, float a, size_t n) { // y = x + a y
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) y[t] = x[t] + a * y[t];
}

// ---- 6: chi at the samples (0 for the samples that take no part) -------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pv_iso(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, PvGrid g,
                                                const float *__restrict__ chi, double *__restrict__ val) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double p[3], nh[3], acc = 0.0;
    if (pv_valid(xyz, nrm, s, p, nh)) {
        const double o[3] = {g.ox, g.oy, g.oz};
        const int N = g.N;
        int i0[3];
        double f[3];
        for (int a = 0; a < 3; a++) {
            const double gq = (p[a] - o[a]) / g.h - 0.5;
            const double fl = floor(gq);
            i0[a] = (int)fl;
            f[a] = gq - fl;
        }
        for (int dz = 0; dz < 2; dz++)
            for (int dy = 0; dy < 2; dy++)
                for (int dx = 0; dx < 2; dx++) {
                    const int i = i0[0] + dx, j = i0[1] + dy, k = i0[2] + dz;
                    if (i < 0 || j < 0 || k < 0 || i >= N || j >= N || k >= N) continue;
                    const double w = ((dx ? f[0] : 1.0 - f[0]) * (dy ? f[1] : 1.0 - f[1])) * (dz ? f[2] : 1.0 - f[2]);
                    acc += w * (double)chi[(size_t)i + (size_t)N * ((size_t)j + (size_t)N * k)];
                }
    }
    val[s] = acc;
}

// ---- 7: marching tetrahedra ---------------------------------------------------------------------------------------------------------
// flag[8 a + d] = the edge (a, d) crosses the surface; the 8th byte of a node stays 0 (one 8-byte store per node)
__global__ __launch_bounds__(256) void k_pv_edge_flags(const float *__restrict__ chi, float iso, int sh, unsigned long long *__restrict__ flag8) {
    const int N = 1 << sh;
    const size_t N3 = (size_t)1 << (3 * sh);
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= N3) return;
    const int i = (int)(a & (N - 1)), j = (int)((a >> sh) & (N - 1)), k = (int)(a >> (2 * sh));
    const bool ia = chi[a] < iso;
    unsigned long long w = 0;
    for (int d = 0; d < 7; d++) {
        const int x = i + c_dir[d][0], y = j + c_dir[d][1], z = k + c_dir[d][2];
        if (x >= N || y >= N || z >= N) continue;
        const bool ib = chi[(size_t)x + (size_t)N * ((size_t)y + (size_t)N * z)] < iso;
        if (ia != ib) w |= 1ull << (8 * d);
    }
    flag8[a] = w;
}

struct U8ToU32 {
    __host__ __device__ unsigned int operator()(uint8_t v) const { return v; }
};

// one vertex per flagged edge, at its rank among the flagged edges (= ascending (a, d)); vkeep (optional) = its cell lies in the mask
__global__ __launch_bounds__(256) void k_pv_emit_vertices(const float *__restrict__ chi, float iso, PvGrid g, const uint8_t *__restrict__ flag,
                                                          const unsigned int *__restrict__ pos, float *__restrict__ verts,
                                                          const uint8_t *__restrict__ mask, uint8_t *__restrict__ vkeep) {
    const int N = g.N, sh = g.sh;
    const size_t N3 = (size_t)1 << (3 * sh);
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= N3) return;
    if (((const unsigned long long *)flag)[a] == 0) return;
    const int ijk[3] = {(int)(a & (N - 1)), (int)((a >> sh) & (N - 1)), (int)(a >> (2 * sh))};
    const double o[3] = {g.ox, g.oy, g.oz};
    const float ca = chi[a];
    for (int d = 0; d < 7; d++) {
        if (!flag[8 * a + d]) continue;
        const size_t b = a + (size_t)c_dir[d][0] + (size_t)N * ((size_t)c_dir[d][1] + (size_t)N * c_dir[d][2]);
        const float cb = chi[b];
        const float t = (iso - ca) / (cb - ca);
        const size_t v = pos[8 * a + d];
        int cell[3];
        for (int c = 0; c < 3; c++) {
            const float pa = (float)(o[c] + ((double)ijk[c] + 0.5) * g.h);
            const float pb = (float)(o[c] + ((double)(ijk[c] + c_dir[d][c]) + 0.5) * g.h);
            const float p = pa + t * (pb - pa);
            verts[3 * v + c] = p;
            const int q = (int)floor(((double)p - o[c]) / g.h);
            cell[c] = q < 0 ? 0 : (q > N - 1 ? N - 1 : q);
        }
        if (vkeep) vkeep[v] = mask[(size_t)cell[0] + (size_t)N * ((size_t)cell[1] + (size_t)N * cell[2])];
    }
}

// faces of a cell (its 000 node is `a`): EMIT = false counts them, true writes them at foff[a] in (tetrahedron, triangle) order
template <bool EMIT>
__global__ __launch_bounds__(256) void k_pv_cell_faces(const float *__restrict__ chi, float iso, int sh, TetTable tab, unsigned int *__restrict__ cnt,
                                                       const unsigned int *__restrict__ foff, const unsigned int *__restrict__ pos,
                                                       int32_t *__restrict__ faces) {
    const int N = 1 << sh;
    const size_t N3 = (size_t)1 << (3 * sh);
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= N3) return;
    const int i = (int)(a & (N - 1)), j = (int)((a >> sh) & (N - 1)), k = (int)(a >> (2 * sh));
    if (i >= N - 1 || j >= N - 1 || k >= N - 1) {
        if (!EMIT) cnt[a] = 0;
        return;
    }
    const size_t st[3] = {1, (size_t)N, (size_t)N * N};
    unsigned int cube = 0; // bit (dx | dy << 1 | dz << 2) = that corner is inside
    for (int c = 0; c < 8; c++)
        if (chi[a + (c & 1) * st[0] + ((c >> 1) & 1) * st[1] + ((c >> 2) & 1) * st[2]] < iso) cube |= 1u << c;
    if (cube == 0 || cube == 255) {
        if (!EMIT) cnt[a] = 0;
        return;
    }
    unsigned int nf = 0;
    size_t o = EMIT ? (size_t)foff[a] : 0;
    for (int t = 0; t < 6; t++) {
        const int pa = c_perm[t][0], pb = c_perm[t][1];
        const int corner[4] = {0, 1 << pa, (1 << pa) | (1 << pb), 7};
        int m = 0;
        for (int v = 0; v < 4; v++) m |= ((cube >> corner[v]) & 1) << v;
        const int nt = tab.ntri[m];
        if (!EMIT) {
            nf += nt;
            continue;
        }
        for (int q = 0; q < nt; q++) {
            int32_t vi[3];
            for (int c = 0; c < 3; c++) {
                const int e = tab.e[m][q][c];
                const int cu = corner[e >> 2], cv = corner[e & 3]; // cu is a subset of cv: the lower node is cu's
                const int d = cv & ~cu;
                const size_t na = a + (cu & 1) * st[0] + ((cu >> 1) & 1) * st[1] + ((cu >> 2) & 1) * st[2];
                vi[c] = (int32_t)pos[8 * na + pv_dir_code(d & 1, (d >> 1) & 1, (d >> 2) & 1)];
            }
            if (c_perm_sign[t] < 0) {
                const int32_t w = vi[1];
                vi[1] = vi[2];
                vi[2] = w;
            }
            faces[3 * o] = vi[0];
            faces[3 * o + 1] = vi[1];
            faces[3 * o + 2] = vi[2];
            o++;
        }
    }
    if (!EMIT) cnt[a] = nf;
}

// ---- 8: trim ------------------------------------------------------------------------------------------------------------------------
// one axis of the Chebyshev dilation: out = max of in over [-r, r] along the axis of stride 1 << (axis * sh)
__global__ __launch_bounds__(256) void k_pv_dilate(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int sh, int axis, int r) {
    const int N = 1 << sh;
    const size_t N3 = (size_t)1 << (3 * sh);
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= N3) return;
    const int c = (int)((a >> (axis * sh)) & (N - 1));
    const size_t st = (size_t)1 << (axis * sh);
    const int lo = c - r < 0 ? 0 : c - r, hi = c + r > N - 1 ? N - 1 : c + r;
    uint8_t m = 0;
    for (int q = lo; q <= hi && !m; q++) m = in[a + (size_t)(q - c) * st] ? 1 : 0; // (q - c may be negative: size_t wraps back, a + ... stays in range)
    out[a] = m;
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

static PvGrid make_grid(const double grid[4], int depth) { return PvGrid{grid[0], grid[1], grid[2], grid[3], depth, 1 << depth}; }

int poisson_rhs_device(const float *d_xyz, const float *d_nrm4, int64_t n, int depth, const double grid[4], float *d_b32, double *d_b64,
                       uint8_t *d_occ, hipStream_t st) {
    const size_t N3 = (size_t)1 << (3 * depth);
    DevMem M;
    unsigned long long *V = M.get<unsigned long long>(3 * N3);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(V, 0, 3 * N3 * sizeof(unsigned long long), st));
    DEVCHK(hipMemsetAsync(d_occ, 0, N3, st));
    const PvGrid g = make_grid(grid, depth);
    hipLaunchKernelGGL(k_pv_splat, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, g, V, d_occ);
    hipLaunchKernelGGL(k_pv_rhs, blocks_for(N3), dim3(256), 0, st, (const long long *)V, depth, d_b32, d_b64);
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    return RSM_OK;
}

namespace {
struct Solver {
    int depth;
    hipStream_t st;
    std::vector<float *> x, b, r; // per level; level 0: x = z, b = the CG residual
    double *part, *scal;
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
    float *z = S.x[0], *r = S.b[0];
    const unsigned rb = red_blocks(N3);
    DEVCHK(hipMemsetAsync(d_chi, 0, N3 * sizeof(float), st));
    DEVCHK(hipMemcpyAsync(r, d_b, N3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    double bb = 0.0;
    hipLaunchKernelGGL(k_pv_dot, dim3(rb), dim3(256), 0, st, d_b, d_b, N3, S.part);
    int s = S.fetch((int)rb, &bb);
    if (s != RSM_OK) return s;
    if (!(bb > 0.0)) return RSM_OK; // b = 0: chi = 0
    const double bnorm = sqrt(bb);
    double rho_old = 0.0;
    int worse = 0;
    bool have_best = true; // (chi = 0, residual 1)
    DEVCHK(hipMemsetAsync(best, 0, N3 * sizeof(float), st));
    *residual = 1.0;
    for (int it = 1; it <= max_cycles; it++) {
        s = S.vcycle(0); // z = M^-1 r
        if (s != RSM_OK) return s;
        double rho = 0.0, pq = 0.0, rr = 0.0;
        hipLaunchKernelGGL(k_pv_dot, dim3(rb), dim3(256), 0, st, r, z, N3, S.part);
        if ((s = S.fetch((int)rb, &rho)) != RSM_OK) return s;
        if (it == 1) DEVCHK(hipMemcpyAsync(p, z, N3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        else hipLaunchKernelGGL(k_pv_xpay, blocks_for(N3), dim3(256), 0, st, p, z, (float)(rho / rho_old), N3);
        hipLaunchKernelGGL(k_pv_stencil<0>, dim3(rb), dim3(256), 0, st, p, (const float *)nullptr, q, depth, S.part);
        if ((s = S.fetch((int)rb, &pq)) != RSM_OK) return s;
        if (pq == 0.0 || !std::isfinite(rho / pq)) break; // nothing left to correct in float32
        hipLaunchKernelGGL(k_pv_axpy, blocks_for(N3), dim3(256), 0, st, d_chi, p, (float)(rho / pq), N3);
        // the residual is recomputed from chi, not updated by recurrence: what is reported is what chi reaches
        hipLaunchKernelGGL(k_pv_stencil<1>, dim3(rb), dim3(256), 0, st, d_chi, d_b, r, depth, S.part);
        if ((s = S.fetch((int)rb, &rr)) != RSM_OK) return s;
        rho_old = rho;
        *cycles = it;
        const double res = sqrt(rr) / bnorm;
        if (history) history[it - 1] = res;
        // float32 conjugate gradients reach a floor (a few 1e-6) and drift away from it afterwards: the best chi is kept, and two cycles
        // in a row without a new best end the solve
        if (res < *residual) {
            *residual = res;
            worse = 0;
            if (res <= rel_residual) break; // (chi is the best iterate)
            DEVCHK(hipMemcpyAsync(best, d_chi, N3 * sizeof(float), hipMemcpyDeviceToDevice, st));
            have_best = true;
        } else if (++worse >= 2)
            break;
    }
    if (*residual > rel_residual && have_best) DEVCHK(hipMemcpyAsync(d_chi, best, N3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    return *residual <= rel_residual ? RSM_OK : RSM_W_NOT_CONVERGED;
}

void poisson_chi_at_samples(const float *d_xyz, const float *d_nrm4, int64_t n, const float *d_chi, int depth, const double grid[4], double *d_val,
                            hipStream_t st) {
    hipLaunchKernelGGL(k_pv_iso, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, d_nrm4, n, make_grid(grid, depth), d_chi, d_val);
}

void poisson_tree_sum(const double *d_v, int64_t n, double *d_part, double *d_sum, hipStream_t st) {
    const unsigned rb = red_blocks((size_t)n);
    hipLaunchKernelGGL(k_pv_sum_f64, dim3(rb), dim3(256), 0, st, d_v, n, d_part);
    hipLaunchKernelGGL(k_pv_sum, dim3(1), dim3(256), 0, st, (const double *)d_part, (int)rb, d_sum);
}

int poisson_iso_device(const float *d_xyz, const float *d_nrm4, int64_t n, int64_t n_valid, const float *d_chi, int depth, const double grid[4],
                       double *iso, hipStream_t st) {
    *iso = 0.0;
    if (n <= 0 || n_valid <= 0) return RSM_OK;
    DevMem M;
    double *val = M.get<double>((size_t)n), *part = M.get<double>(PV_RED_BLOCKS), *scal = M.get<double>(1);
    if (!M.ok) return RSM_E_NOMEM;
    poisson_chi_at_samples(d_xyz, d_nrm4, n, d_chi, depth, grid, val, st);
    poisson_tree_sum(val, n, part, scal, st);
    double sum = 0.0;
    DEVCHK(hipMemcpyAsync(&sum, scal, sizeof sum, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    *iso = sum / (double)n_valid;
    return RSM_OK;
}

// step 8's second half, for the dense extraction and the banded one (k_poisson_band.hip): of `full` (its vertices flagged by vkeep) the faces whose
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
    poisson_mesh_free(out);
    untrimmed[0] = untrimmed[1] = 0;
    const size_t N3 = (size_t)1 << (3 * depth);
    const PvGrid g = make_grid(grid, depth);
    const float iso32 = (float)iso;
    const TetTable tab = make_tet_table();
    DevMem M;
    uint8_t *flag = (uint8_t *)M.get<unsigned long long>(N3);
    unsigned int *pos = M.get<unsigned int>(8 * N3);
    unsigned int *cnt = M.get<unsigned int>(N3), *foff = M.get<unsigned int>(N3);
    if (!M.ok) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_pv_edge_flags, blocks_for(N3), dim3(256), 0, st, d_chi, iso32, depth, (unsigned long long *)flag);
    int s = scan_u32(M, rocprim::make_transform_iterator((const uint8_t *)flag, U8ToU32()), pos, 8 * N3, st);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL(k_pv_cell_faces<false>, blocks_for(N3), dim3(256), 0, st, d_chi, iso32, depth, tab, cnt, (const unsigned int *)nullptr,
                       (const unsigned int *)nullptr, (int32_t *)nullptr);
    if ((s = scan_u32(M, (const unsigned int *)cnt, foff, N3, st)) != RSM_OK) return s;
    uint64_t nv = 0, nf = 0;
    // (the last node has no edge toward higher indices and is no cell: both last flags are 0, the totals are the last positions)
    if ((s = scan_total(flag + 8 * N3 - 1, pos + 8 * N3 - 1, 1, st, &nv)) != RSM_OK) return s;
    if ((s = scan_total(cnt + N3 - 1, foff + N3 - 1, 1, st, &nf)) != RSM_OK) return s;
    DEVCHK(hipGetLastError());
    untrimmed[0] = (int64_t)nv;
    untrimmed[1] = (int64_t)nf;
    if (nv == 0 || nf == 0) return RSM_OK;
    if (nv > (uint64_t)INT32_MAX || nf > (uint64_t)INT32_MAX / 3) return RSM_E_NOMEM;
    float *verts = nullptr;
    int32_t *faces = nullptr;
    if (hipMalloc((void **)&verts, nv * 3 * sizeof(float)) != hipSuccess) return RSM_E_NOMEM;
    if (hipMalloc((void **)&faces, nf * 3 * sizeof(int32_t)) != hipSuccess) {
        (void)hipFree(verts);
        return RSM_E_NOMEM;
    }
    PoissonMesh full;
    full.d_v = verts;
    full.d_f = faces;
    full.nv = (int64_t)nv;
    full.nf = (int64_t)nf;
    const bool trim = trim_cells > 0 && d_occ;
    uint8_t *mask = nullptr, *vkeep = nullptr;
    if (trim) {
        uint8_t *t0 = M.get<uint8_t>(N3), *t1 = M.get<uint8_t>(N3);
        vkeep = M.get<uint8_t>(nv);
        if (!M.ok) {
            poisson_mesh_free(&full);
            return RSM_E_NOMEM;
        }
        hipLaunchKernelGGL(k_pv_dilate, blocks_for(N3), dim3(256), 0, st, d_occ, t0, depth, 0, trim_cells);
        hipLaunchKernelGGL(k_pv_dilate, blocks_for(N3), dim3(256), 0, st, (const uint8_t *)t0, t1, depth, 1, trim_cells);
        hipLaunchKernelGGL(k_pv_dilate, blocks_for(N3), dim3(256), 0, st, (const uint8_t *)t1, t0, depth, 2, trim_cells);
        mask = t0;
    }
    hipLaunchKernelGGL(k_pv_emit_vertices, blocks_for(N3), dim3(256), 0, st, d_chi, iso32, g, (const uint8_t *)flag, (const unsigned int *)pos, verts,
                       (const uint8_t *)mask, vkeep);
    hipLaunchKernelGGL(k_pv_cell_faces<true>, blocks_for(N3), dim3(256), 0, st, d_chi, iso32, depth, tab, (unsigned int *)nullptr,
                       (const unsigned int *)foff, (const unsigned int *)pos, faces);
    if (!trim) {
        if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
            poisson_mesh_free(&full);
            return RSM_E_HIP;
        }
        *out = full;
        return RSM_OK;
    }
    return poisson_trim_commit(M, full, vkeep, out, st);
}
