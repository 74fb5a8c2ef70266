// k_meshfill.hip -- fills the vertices no view sees (best_view < 0) with the harmonic extension of the colours around them, so that the
// coloured mesh is coloured everywhere as TextureStitcher's is.  Not a port (no source in the reference tree): every rule is
// defined in DESIGN.md 9 (f18) and restated in numpy in tests/meshfill_restatement.py, and the kernels are held to that restatement exactly.
//   neighbours      mesh_common.h's neighbour CSR over the corner lists (k_mesh_nbr_csr): every neighbour, known or not, in f10's order
//   front           round r = 1, 2, ...: an unknown vertex without a level takes the mean of its incidences of level < r, in order, and the
//                   level r.  In place, no atomics on the values: a level written in this launch reads as UNREACHED or r, both fail < r, and
//                   the rows read were written by an earlier launch.  A thread per unknown vertex (a list compacted once); rounds go out
//                   in batches and one counter, the largest level, comes back per batch: a round that reaches nothing is a no-op    k_mf_front
//   system          per channel over the filled vertices (1 <= level <= L): sum over the incidences to known or filled neighbours of
//                   (x_i - x_j) = 0; the incidences to unreached neighbours (at the cap of the rounds only) are dropped        k_mf_deg
//   solver          f10's Jacobi-preconditioned Chebyshev iteration on the interval [1 / (2 (L + 1))^2, 2], a fixed number of steps,
//                   coefficients from the host (mesh_common.h: ChebSchedule): one launch per step, a thread per filled vertex (a list
//                   compacted once), x ping-pong over all rows (the others are copied into both buffers once), d in place     k_mf_step
//   bytes           clamp(floor(x + 0.5), 0, 255) for the filled vertices; the largest |x - x_front| by an integer atomicMax   k_mf_bytes
// No float atomics.  Built with -ffp-contract=off (csrc/Makefile): every expression below is evaluated as written.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"

#include <math.h>
#include <string.h>

#include <algorithm>

namespace {

typedef unsigned long long u64;

#define MF_UNREACHED 0x7fffffff // the level of an unknown vertex no round has reached (-1 outside this unit)

enum { C_L = 0, C_INC, C_DMAX, C_CLAMP, C_MAXDIFF, C_N };

// a level may be written by another thread of the same launch: one aligned 32-bit access either way
__device__ __forceinline__ int32_t lv_load(const int32_t *level, size_t i) { return __hip_atomic_load(level + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lv_store(int32_t *level, size_t i, int32_t v) { __hip_atomic_store(level + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// (a stale read only costs an atomic that changes nothing)
__device__ __forceinline__ void max_if(u64 v, u64 *ctr) {
    if (v > __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(ctr, v);
}

// ---- known and unknown ------------------------------------------------------------------------------------------------------------------
// level 0 / UNREACHED by best_view's sign, x = the bytes as doubles, unknown[i] = 1 for an unknown vertex
__global__ __launch_bounds__(256) void k_mf_init(size_t nv, const int32_t *__restrict__ best, const uint8_t *__restrict__ rgb, int32_t *__restrict__ level,
                                                 double *__restrict__ x, uint32_t *__restrict__ unknown) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const bool known = best[i] >= 0;
    level[i] = known ? 0 : MF_UNREACHED;
    unknown[i] = known ? 0u : 1u;
    for (int k = 0; k < 3; k++) x[3 * i + k] = (double)rgb[3 * i + k];
}
// a caller's levels (the solve stage): 0 known, 1 .. L filled, anything else unreached; filled[i] = 1 for a filled vertex
__global__ __launch_bounds__(256) void k_mf_level_in(size_t nv, const int32_t *__restrict__ in, int32_t L, int32_t *__restrict__ level, uint32_t *__restrict__ filled) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int32_t v = in[i];
    const bool fill = v >= 1 && v <= L;
    level[i] = v == 0 ? 0 : fill ? v : MF_UNREACHED;
    filled[i] = fill ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_mf_level_out(size_t nv, const int32_t *__restrict__ level, int32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nv) out[i] = level[i] == MF_UNREACHED ? -1 : level[i];
}
__global__ __launch_bounds__(256) void k_mf_flag_filled(size_t nv, const int32_t *__restrict__ level, uint32_t *__restrict__ filled) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nv) filled[i] = (level[i] != 0 && level[i] != MF_UNREACHED) ? 1u : 0u;
}
// list = the flagged vertices, ascending (pos: the exclusive scan of flag)
__global__ __launch_bounds__(256) void k_mf_scatter(size_t nv, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, uint32_t *__restrict__ list) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nv && flag[i]) list[pos[i]] = (uint32_t)i;
}

// ---- the front --------------------------------------------------------------------------------------------------------------------------
// round r over the n unknown vertices of list; level and x are read and written here (never the same row: see the head of the file)
__global__ __launch_bounds__(256) void k_mf_front(const uint32_t *__restrict__ list, size_t n, int32_t r, const uint32_t *__restrict__ row,
                                                  const uint32_t *__restrict__ nbr, int32_t *level, double *x, u64 *__restrict__ ctr) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t i = list[t];
    if (lv_load(level, i) < r) return;
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    uint32_t k = 0;
    for (size_t e = 2 * (size_t)row[i], end = 2 * (size_t)row[i + 1]; e < end; e++) {
        const size_t j = nbr[e];
        if (lv_load(level, j) < r) {
            S0 = S0 + x[3 * j];
            S1 = S1 + x[3 * j + 1];
            S2 = S2 + x[3 * j + 2];
            k++;
        }
    }
    if (!k) return;
    const double kd = (double)k;
    x[3 * i] = S0 / kd;
    x[3 * i + 1] = S1 / kd;
    x[3 * i + 2] = S2 / kd;
    lv_store(level, i, r);
    max_if((u64)r, ctr + C_L);
}

// ---- the system and the solver ------------------------------------------------------------------------------------------------------------
// CAPPED: a filled vertex may have unreached neighbours (the rounds stopped at the cap; a caller's levels), whose incidences are dropped;
// otherwise every neighbour of a filled vertex is known or filled and no level is read
template <bool CAPPED>
__device__ __forceinline__ bool mf_kept(const int32_t *__restrict__ level, size_t j) {
    return !CAPPED || level[j] != MF_UNREACHED;
}
// per filled vertex list[t]: deg[t] = its kept incidences, x0[t] = the front's value, d[t] = 0
template <bool CAPPED>
__global__ __launch_bounds__(256) void k_mf_deg(const uint32_t *__restrict__ list, size_t n, const uint32_t *__restrict__ row, const uint32_t *__restrict__ nbr,
                                                const int32_t *__restrict__ level, const double *__restrict__ x, uint32_t *__restrict__ deg, double *__restrict__ x0,
                                                double *__restrict__ d, u64 *__restrict__ ctr) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t i = list[t];
    uint32_t k = 0;
    for (size_t e = 2 * (size_t)row[i], end = 2 * (size_t)row[i + 1]; e < end; e++)
        if (mf_kept<CAPPED>(level, nbr[e])) k++;
    deg[t] = k;
    for (int c = 0; c < 3; c++) {
        x0[3 * t + c] = x[3 * i + c];
        d[3 * t + c] = 0.0;
    }
    if (k) atomicAdd(ctr + C_INC, (u64)k);
    max_if((u64)k, ctr + C_DMAX);
}
// one Chebyshev step, a thread per filled vertex: S = sum of (x_i - x_j), z = (0 - S) / deg, d = alpha d + beta z, x' = x + d.  A filled
// vertex without a kept incidence (a caller's levels only) has z = 0
template <bool CAPPED>
__global__ __launch_bounds__(256) void k_mf_step(const uint32_t *__restrict__ list, size_t n, const uint32_t *__restrict__ row, const uint32_t *__restrict__ nbr,
                                                 const int32_t *__restrict__ level, const uint32_t *__restrict__ deg, const double *__restrict__ x,
                                                 double *__restrict__ d, double *__restrict__ xo, double alpha, double beta) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t i = list[t];
    const double x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2];
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    for (size_t e = 2 * (size_t)row[i], end = 2 * (size_t)row[i + 1]; e < end; e++) {
        const size_t j = nbr[e];
        if (!mf_kept<CAPPED>(level, j)) continue;
        S0 = S0 + (x0 - x[3 * j]);
        S1 = S1 + (x1 - x[3 * j + 1]);
        S2 = S2 + (x2 - x[3 * j + 2]);
    }
    const uint32_t k = deg[t];
    const double kd = (double)k;
    const double z0 = k ? (0.0 - S0) / kd : 0.0, z1 = k ? (0.0 - S1) / kd : 0.0, z2 = k ? (0.0 - S2) / kd : 0.0;
    const double d0 = (alpha * d[3 * t]) + (beta * z0), d1 = (alpha * d[3 * t + 1]) + (beta * z1), d2 = (alpha * d[3 * t + 2]) + (beta * z2);
    d[3 * t] = d0;
    d[3 * t + 1] = d1;
    d[3 * t + 2] = d2;
    xo[3 * i] = x0 + d0;
    xo[3 * i + 1] = x1 + d1;
    xo[3 * i + 2] = x2 + d2;
}

// ---- the bytes ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mf_bytes(const uint32_t *__restrict__ list, size_t n, const double *__restrict__ x, const double *__restrict__ x0,
                                                  uint8_t *__restrict__ rgb, u64 *__restrict__ ctr) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const size_t i = list[t];
    u64 clamped = 0;
    double big = 0.0;
    for (int k = 0; k < 3; k++) {
        const double v = x[3 * i + k], diff = fabs(v - x0[3 * t + k]);
        big = diff > big ? diff : big;
        double q = floor(v + 0.5);
        if (!(q >= 0.0 && q <= 255.0)) {
            clamped++;
            q = q > 255.0 ? 255.0 : 0.0;
        }
        rgb[3 * i + k] = (uint8_t)(int)q;
    }
    if (clamped) atomicAdd(ctr + C_CLAMP, clamped);
    // (doubles >= 0 order as their bit patterns)
    max_if((u64)__double_as_longlong(big), ctr + C_MAXDIFF);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// everything a call needs, allocated before anything is enqueued (mesh_common.h: a hipMalloc once work is on the stream costs the call time)
struct Fill {
    size_t nv = 0;
    uint32_t *row = nullptr, *corner = nullptr, *nbr = nullptr;
    int32_t *level = nullptr;
    double *xa = nullptr, *xb = nullptr, *d = nullptr, *x0 = nullptr;
    uint32_t *flag = nullptr, *pos = nullptr, *list = nullptr, *deg = nullptr;
    u64 *ctr = nullptr;
    ScanTmp scan;
};

int fill_setup(DevMem &M, Fill &F, const int32_t *d_f, size_t nv, size_t nf, bool solver, hipStream_t st) {
    F.nv = nv;
    F.level = M.get<int32_t>(nv);
    F.xa = M.get<double>(3 * nv);
    F.flag = M.get<uint32_t>(nv);
    F.pos = M.get<uint32_t>(nv);
    F.list = M.get<uint32_t>(nv);
    F.nbr = M.get<uint32_t>(6 * nf);
    F.ctr = M.get<u64>(C_N);
    if (solver) {
        F.xb = M.get<double>(3 * nv);
        F.d = M.get<double>(3 * nv);
        F.x0 = M.get<double>(3 * nv);
        F.deg = M.get<uint32_t>(nv);
    }
    if (!M.ok) return RSM_E_NOMEM;
    const int s = mesh_corner_lists(M, d_f, nv, nf, &F.row, &F.corner, st);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL(k_mesh_nbr_csr<>, blocks_for(nv), dim3(256), 0, st, nv, d_f, (const uint32_t *)F.row, (const uint32_t *)F.corner, F.nbr);
    DEVCHK(hipMemsetAsync(F.ctr, 0, C_N * sizeof(u64), st));
    return RSM_OK;
}

// list = the vertices of flag, *total of them (one host round trip)
int compact(DevMem &M, Fill &F, uint64_t *total, hipStream_t st) {
    const int s = scan_u32(M, (const uint32_t *)F.flag, F.pos, F.nv, st, &F.scan);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL(k_mf_scatter, blocks_for(F.nv), dim3(256), 0, st, F.nv, (const uint32_t *)F.flag, (const uint32_t *)F.pos, F.list);
    return scan_total(F.flag, F.pos, F.nv, st, total);
}

// the rounds over the nu unknown vertices of F.list, `batch` of them between two read-backs of the largest level; *L = the largest level reached
int front(Fill &F, size_t nu, int max_rounds, int batch, int *L, hipStream_t st) {
    int r = 0;
    *L = 0;
    for (;;) {
        int n = batch;
        if (max_rounds > 0) n = std::min(n, max_rounds - r);
        if (n <= 0) break;
        for (int k = 0; k < n; k++)
            hipLaunchKernelGGL(k_mf_front, blocks_for(nu), dim3(256), 0, st, (const uint32_t *)F.list, nu, (int32_t)++r, (const uint32_t *)F.row, (const uint32_t *)F.nbr,
                               F.level, F.xa, F.ctr);
        u64 h = 0;
        DEVCHK(hipMemcpyAsync(&h, F.ctr + C_L, sizeof h, hipMemcpyDeviceToHost, st));
        DEVCHK(hipStreamSynchronize(st));
        DEVCHK(hipGetLastError());
        *L = (int)h;
        if (*L < r) break; // a round reached nothing: so would every later one
    }
    return RSM_OK;
}

// `steps` steps over the n filled vertices of F.list from F.xa; *x = the buffer that holds the result.  Enqueues only
template <bool CAPPED>
int solve_t(Fill &F, size_t n, int L, int steps, double **x, hipStream_t st) {
    hipLaunchKernelGGL(k_mf_deg<CAPPED>, blocks_for(n), dim3(256), 0, st, (const uint32_t *)F.list, n, (const uint32_t *)F.row, (const uint32_t *)F.nbr,
                       (const int32_t *)F.level, (const double *)F.xa, F.deg, F.x0, F.d, F.ctr);
    double *xa = F.xa, *xb = F.xb;
    if (steps > 0) DEVCHK(hipMemcpyAsync(xb, xa, sizeof(double) * 3 * F.nv, hipMemcpyDeviceToDevice, st));
    const double w = 2.0 * ((double)L + 1.0);
    ChebSchedule cheb(1.0 / (w * w));
    for (int k = 0; k < steps; k++) {
        double alpha, beta;
        cheb.step(k, &alpha, &beta);
        hipLaunchKernelGGL(k_mf_step<CAPPED>, blocks_for(n), dim3(256), 0, st, (const uint32_t *)F.list, n, (const uint32_t *)F.row, (const uint32_t *)F.nbr,
                           (const int32_t *)F.level, (const uint32_t *)F.deg, (const double *)xa, F.d, xb, alpha, beta);
        std::swap(xa, xb);
    }
    *x = xa;
    return RSM_OK;
}
int solve(Fill &F, size_t n, int L, int steps, bool capped, double **x, hipStream_t st) {
    return capped ? solve_t<true>(F, n, L, steps, x, st) : solve_t<false>(F, n, L, steps, x, st);
}

} // namespace

int mesh_fill_steps(int L, double reduction) {
    const double w = 2.0 * ((double)L + 1.0);
    return cheb_steps(1.0 / (w * w), reduction, RSM_MESH_FILL_MAX_ITERATIONS);
}

int mesh_fill_front_device(const int32_t *d_f, int64_t nv_, int64_t nf_, const int32_t *d_best, const uint8_t *d_rgb, int max_rounds, int batch, double *d_x,
                           int32_t *d_level, int *L, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    *L = 0;
    int s = mesh_validate_device(nullptr, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK || nv == 0) return s;
    DevMem M;
    Fill F;
    if ((s = fill_setup(M, F, d_f, nv, nf, false, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_mf_init, blocks_for(nv), dim3(256), 0, st, nv, d_best, d_rgb, F.level, F.xa, F.flag);
    uint64_t nu = 0;
    if ((s = compact(M, F, &nu, st)) != RSM_OK) return s;
    if (nu > 0 && nu < nv && (s = front(F, (size_t)nu, max_rounds, batch, L, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_mf_level_out, blocks_for(nv), dim3(256), 0, st, nv, (const int32_t *)F.level, d_level);
    DEVCHK(hipMemcpyAsync(d_x, F.xa, sizeof(double) * 3 * nv, hipMemcpyDeviceToDevice, st));
    return mesh_finish(st);
}

int mesh_fill_solve_device(const int32_t *d_f, int64_t nv_, int64_t nf_, const int32_t *d_level, int L, int iterations, double *d_x, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    int s = mesh_validate_device(nullptr, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK || nv == 0) return s;
    DevMem M;
    Fill F;
    if ((s = fill_setup(M, F, d_f, nv, nf, true, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_mf_level_in, blocks_for(nv), dim3(256), 0, st, nv, d_level, (int32_t)L, F.level, F.flag);
    DEVCHK(hipMemcpyAsync(F.xa, d_x, sizeof(double) * 3 * nv, hipMemcpyDeviceToDevice, st));
    uint64_t n = 0;
    if ((s = compact(M, F, &n, st)) != RSM_OK) return s;
    if (n == 0) return mesh_finish(st);
    double *x = nullptr;
    if ((s = solve(F, (size_t)n, L, iterations, true, &x, st)) != RSM_OK) return s;
    DEVCHK(hipMemcpyAsync(d_x, x, sizeof(double) * 3 * nv, hipMemcpyDeviceToDevice, st));
    return mesh_finish(st);
}

int mesh_fill_device(const int32_t *d_f, int64_t nv_, int64_t nf_, const int32_t *d_best, uint8_t *d_rgb, int32_t *d_level, const rsm_mesh_fill_params *p, int batch,
                     double *stats, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    double S[RSM_MESH_FILL_STATS] = {0};
    S[0] = (double)nv;
    int s = mesh_validate_device(nullptr, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK) return s;
    if (nv > 0) {
        DevMem M;
        Fill F;
        if ((s = fill_setup(M, F, d_f, nv, nf, true, st)) != RSM_OK) return s;
        hipLaunchKernelGGL(k_mf_init, blocks_for(nv), dim3(256), 0, st, nv, d_best, (const uint8_t *)d_rgb, F.level, F.xa, F.flag);
        uint64_t nu = 0, n = 0;
        if ((s = compact(M, F, &nu, st)) != RSM_OK) return s;
        int L = 0;
        if (nu > 0 && nu < nv) {
            if ((s = front(F, (size_t)nu, p->max_rounds, batch, &L, st)) != RSM_OK) return s;
            if (L > 0) {
                hipLaunchKernelGGL(k_mf_flag_filled, blocks_for(nv), dim3(256), 0, st, nv, (const int32_t *)F.level, F.flag);
                if ((s = compact(M, F, &n, st)) != RSM_OK) return s;
            }
        }
        S[1] = (double)(nv - nu);
        S[2] = (double)n;
        S[3] = (double)(nu - n);
        S[4] = (double)L;
        if (n > 0) {
            int steps = p->iterations;
            if (steps == 0 && (steps = mesh_fill_steps(L, p->reduction)) < 0) {
                *invalid = 4;
                return RSM_E_INVALID;
            }
            double *x = nullptr;
            if ((s = solve(F, (size_t)n, L, steps, p->max_rounds > 0 && L == p->max_rounds, &x, st)) != RSM_OK) return s;
            hipLaunchKernelGGL(k_mf_bytes, blocks_for((size_t)n), dim3(256), 0, st, (const uint32_t *)F.list, (size_t)n, (const double *)x, (const double *)F.x0, d_rgb,
                               F.ctr);
            u64 h[C_N];
            DEVCHK(hipMemcpyAsync(h, F.ctr, sizeof h, hipMemcpyDeviceToHost, st));
            DEVCHK(hipStreamSynchronize(st));
            DEVCHK(hipGetLastError());
            S[5] = (double)h[C_INC];
            S[6] = (double)h[C_DMAX];
            S[7] = (double)steps;
            S[8] = (double)h[C_CLAMP];
            S[9] = __builtin_bit_cast(double, h[C_MAXDIFF]);
        }
        if (d_level) hipLaunchKernelGGL(k_mf_level_out, blocks_for(nv), dim3(256), 0, st, nv, (const int32_t *)F.level, d_level);
        if ((s = mesh_finish(st)) != RSM_OK) return s; // (the scratch goes with M: nothing of it may still be in use)
    }
    if (stats) memcpy(stats, S, sizeof S);
    return RSM_OK;
}
