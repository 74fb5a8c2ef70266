// poisson_space.h -- the node space of the Poisson surface and the rules stated once over it: what the
// dense grid (k_poisson.hip; f7), the density-adaptive splat (k_poisson_density.hip; f14), the band of bricks (k_poisson_band.hip; f16) and the
// two together (k_poisson_band_density.hip; f17) share.  The grid of a call is mesh_common.h's MtGrid.  A node space answers three questions:
//   elem(i, j, k)        the element of node (i, j, k): >= 0, -1 inactive (the band only), -2 outside the grid
//   at(a) / coords       a node's place from its element
//   nbr(at, dx, dy, dz)  the element of its neighbour at an offset in -1..1 per axis, with elem's three answers
// DenseSpace is index arithmetic on 2^sh nodes per axis; BandSpace goes through the slot table and, per node, the slot's 27 neighbour slots.
// The kernels are templates for the reason dev_prims.h gives.  Every unit that includes this is built with -ffp-contract=off.
#pragma once

#include "mesh_common.h"
#include "rsm_dev.h"

#include <cmath>

#define PV_FIX 4294967296.0 // 2^32: the splat's fixed-point scale
#define PB_NODES 512        // nodes of a brick

static inline MtGrid pv_grid(const double grid[4], int depth) { return MtGrid{grid[0], grid[1], grid[2], grid[3], 1 << depth}; }

// ---- the dense grid: element = i + N (j + N k) ----------------------------------------------------------------------------------------
struct DenseSpace {
    int sh; // N = 1 << sh nodes per axis
    struct At {
        size_t a;
        int i, j, k;
    };
    __host__ __device__ size_t nodes() const { return (size_t)1 << (3 * sh); }
    __device__ __forceinline__ long long elem(int i, int j, int k) const {
        const unsigned N = 1u << sh;
        if ((unsigned)i >= N || (unsigned)j >= N || (unsigned)k >= N) return -2;
        return (long long)(((((size_t)k << sh) + (size_t)j) << sh) + (size_t)i);
    }
    __device__ __forceinline__ At at(size_t a) const {
        const int m = (1 << sh) - 1;
        return At{a, (int)(a & m), (int)((a >> sh) & m), (int)(a >> (2 * sh))};
    }
    __device__ __forceinline__ void coords(const At &n, int ijk[3]) const { ijk[0] = n.i, ijk[1] = n.j, ijk[2] = n.k; }
    __device__ __forceinline__ long long nbr(const At &n, int dx, int dy, int dz) const { return elem(n.i + dx, n.j + dy, n.k + dz); }
};

// ---- the band of bricks as a kernel sees it (what a kernel needs of a PoissonBand): brick-major, element slot * 512 + lx + 8 (ly + 8 lz) -------
struct PbBand {
    const int32_t *slot, *active, *nbr;
    int sh, bsh, N; // N = 1 << sh nodes, 1 << bsh bricks per axis
};
// the slot of the brick that holds node (i, j, k): -1 inactive, -2 outside the grid
__device__ __forceinline__ int pb_slot_of(const PbBand &B, int i, int j, int k) {
    if ((unsigned)i >= (unsigned)B.N || (unsigned)j >= (unsigned)B.N || (unsigned)k >= (unsigned)B.N) return -2;
    return B.slot[(size_t)(i >> 3) + (((size_t)(j >> 3) + ((size_t)(k >> 3) << B.bsh)) << B.bsh)];
}
__device__ __forceinline__ int pb_local(int i, int j, int k) { return (i & 7) + 8 * ((j & 7) + 8 * (k & 7)); }
// ... and the node's element, or the negative slot
__device__ __forceinline__ long long pb_elem_of(const PbBand &B, int i, int j, int k) {
    const int s = pb_slot_of(B, i, j, k);
    return s < 0 ? (long long)s : (long long)s * PB_NODES + pb_local(i, j, k);
}
// from a slot's 27 neighbour slots nb[(cx + 1) + 3 ((cy + 1) + 3 (cz + 1))]: the element of its node at local (x, y, z), each in -1 .. 8
__device__ __forceinline__ long long pb_node(const int32_t *nb, int x, int y, int z) {
    const int s = nb[((x >> 3) + 1) + 3 * (((y >> 3) + 1) + 3 * ((z >> 3) + 1))];
    return s < 0 ? (long long)s : (long long)s * PB_NODES + pb_local(x, y, z);
}
// the grid coordinates of a slot's node 0
__device__ __forceinline__ void pb_origin(const PbBand &B, int slot, int o[3]) {
    const int b = B.active[slot], m = (1 << B.bsh) - 1;
    o[0] = (b & m) << 3;
    o[1] = ((b >> B.bsh) & m) << 3;
    o[2] = (b >> (2 * B.bsh)) << 3;
}
// the band as a node space (the solver's kernels take the PbBand alone)
struct BandSpace {
    PbBand B;
    size_t n_nodes;
    struct At {
        const int32_t *nb; // the 27 neighbour slots of the node's slot
        int slot, x, y, z; // the node's local coordinates
    };
    __host__ __device__ size_t nodes() const { return n_nodes; }
    __device__ __forceinline__ long long elem(int i, int j, int k) const { return pb_elem_of(B, i, j, k); }
    __device__ __forceinline__ At at(size_t a) const {
        const int l = (int)(a & 511);
        return At{B.nbr + (a >> 9) * 27, (int)(a >> 9), l & 7, (l >> 3) & 7, l >> 6};
    }
    __device__ __forceinline__ void coords(const At &n, int ijk[3]) const {
        pb_origin(B, n.slot, ijk);
        ijk[0] += n.x, ijk[1] += n.y, ijk[2] += n.z;
    }
    __device__ __forceinline__ long long nbr(const At &n, int dx, int dy, int dz) const { return pb_node(n.nb, n.x + dx, n.y + dy, n.z + dz); }
};

static inline size_t pb_nodes(const PoissonBand &b) { return (size_t)b.n_active * PB_NODES; }
static inline PbBand pb_band(const PoissonBand &b) { return PbBand{b.d_slot, b.d_active, b.d_nbr, b.depth, b.depth - 3, 1 << b.depth}; }
static inline BandSpace pb_space(const PoissonBand &b) { return BandSpace{pb_band(b), pb_nodes(b)}; }

// ---- the sample's cell ---------------------------------------------------------------------------------------------------------------------
// mesh_common.h's mt_cell / mt_weight / mt_cell_index are the trilinear cell.  The occupancy cell of a coordinate, clamped to the grid; the
// compare in double is defined for every input (NaN lands on 0)
__device__ __forceinline__ int pv_occ_cell(double x, double o, double h, int N) {
    const double u = floor((x - o) / h);
    return u >= 0.0 ? (u < (double)N ? (int)u : N - 1) : 0;
}
__device__ __forceinline__ void pv_occ_cell3(const double p[3], const MtGrid &g, int c[3]) {
    c[0] = pv_occ_cell(p[0], g.ox, g.h, g.N), c[1] = pv_occ_cell(p[1], g.oy, g.h, g.N), c[2] = pv_occ_cell(p[2], g.oz, g.h, g.N);
}

// ---- the eight-node splat of one sample: V[a][node] += llrint((wt (alpha n^_a)) 2^32) at the nodes of its cell that lie in the space; 64-bit
// integer atomics, so no order in the sum; a zero term is skipped.  an = alpha n^; V's components are `stride` words apart -------------------
template <class Space>
__device__ __forceinline__ void pv_splat8(const Space &S, const double p[3], const MtGrid &g, const double an[3], unsigned long long *__restrict__ V, size_t stride) {
    double fl[3], f[3];
    int i0[3];
    mt_cell(p, g, fl, f);
    if (!mt_cell_index(fl, g.N, i0)) return;
    for (int dz = 0; dz < 2; dz++)
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const long long node = S.elem(i0[0] + dx, i0[1] + dy, i0[2] + dz);
                if (node < 0) continue; // outside the grid; (inactive cannot happen with band_bricks >= 1)
                const double wt = mt_weight(f, dx, dy, dz);
                for (int a = 0; a < 3; a++) {
                    const long long q = __double2ll_rn((wt * an[a]) * PV_FIX);
                    if (q) atomicAdd(&V[a * stride + (size_t)node], (unsigned long long)q);
                }
            }
}

// ---- chi at the samples (0 for the samples that take no part) --------------------------------------------------------------------------------
template <class Space>
__global__ __launch_bounds__(256) void k_pv_chi_at_samples(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, MtGrid g, Space S,
                                                           const float *__restrict__ chi, double *__restrict__ val) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double p[3], nh[3], acc = 0.0;
    if (pv_valid(xyz, nrm, s, p, nh)) {
        double fl[3], f[3];
        int i0[3];
        mt_cell(p, g, fl, f);
        if (mt_cell_index(fl, g.N, i0))
            for (int dz = 0; dz < 2; dz++)
                for (int dy = 0; dy < 2; dy++)
                    for (int dx = 0; dx < 2; dx++) {
                        const long long e = S.elem(i0[0] + dx, i0[1] + dy, i0[2] + dz);
                        if (e < 0) continue;
                        acc += mt_weight(f, dx, dy, dz) * (double)chi[e];
                    }
    }
    val[s] = acc;
}

// ---- the right-hand side: 1/2 central differences of the splat (0 outside the space).  Word = long long: exact in integers, then one
// conversion and the fixed-point scale; double: the cascade's field as it is ---------------------------------------------------------------------
__device__ __forceinline__ double pv_rhs_of(long long dx, long long dy, long long dz) { return (0.5 * (((double)dx + (double)dy) + (double)dz)) / PV_FIX; }
__device__ __forceinline__ double pv_rhs_of(double dx, double dy, double dz) { return 0.5 * ((dx + dy) + dz); }
template <class Word>
__device__ __forceinline__ Word pv_word(const Word *__restrict__ C, long long e) { return e < 0 ? (Word)0 : C[e]; }
template <class Space, class Word>
__global__ __launch_bounds__(256) void k_pv_rhs(const Word *__restrict__ V, Space S, float *__restrict__ b32, double *__restrict__ b64) {
    const size_t nodes = S.nodes();
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nodes) return;
    const auto n = S.at(t);
    const Word *Vx = V, *Vy = V + nodes, *Vz = V + 2 * nodes;
    const Word dx = pv_word(Vx, S.nbr(n, 1, 0, 0)) - pv_word(Vx, S.nbr(n, -1, 0, 0));
    const Word dy = pv_word(Vy, S.nbr(n, 0, 1, 0)) - pv_word(Vy, S.nbr(n, 0, -1, 0));
    const Word dz = pv_word(Vz, S.nbr(n, 0, 0, 1)) - pv_word(Vz, S.nbr(n, 0, 0, -1));
    const double b = pv_rhs_of(dx, dy, dz);
    if (b32) b32[t] = (float)b;
    if (b64) b64[t] = b;
}

// ---- f14's prolongation at one node: cell-centred trilinear, x, then y, for the near and the far z-plane, 0.75 near + 0.25 far.  A(i, j, k) reads
// the coarse field (0 outside it); ci / cj / ck = the near and the far coarse node per axis ------------------------------------------------------
template <class Coarse>
__device__ __forceinline__ double pd_prolong_at(Coarse A, const int ci[2], const int cj[2], const int ck[2]) {
    double y[2];
    for (int c = 0; c < 2; c++) {
        const double x0 = 0.75 * A(ci[0], cj[0], ck[c]) + 0.25 * A(ci[1], cj[0], ck[c]);
        const double x1 = 0.75 * A(ci[0], cj[1], ck[c]) + 0.25 * A(ci[1], cj[1], ck[c]);
        y[c] = 0.75 * x0 + 0.25 * x1;
    }
    return 0.75 * y[0] + 0.25 * y[1];
}

// ---- what the solvers share besides their own kernels ------------------------------------------------------------------------------------------
template <int = 0>
__global__ __launch_bounds__(256) void k_pv_axpy(float *__restrict__ y, const float *__restrict__ x, float a, size_t n) { // y += a x
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) y[t] = y[t] + a * x[t];
}
template <int = 0>
__global__ __launch_bounds__(256) void k_pv_xpay(float *__restrict__ y, const float *__restrict__ x, float a, size_t n) { // y = x + a y
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) y[t] = x[t] + a * y[t];
}
// one axis of the Chebyshev dilation on a dense lattice of 1 << sh per axis (the cells of the dense grid, the bricks of a band): out = max of in
// over [-r, r] along the axis of stride 1 << (axis * sh)
template <int = 0>
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

// ---- host: the float32 conjugate gradients of both solves --------------------------------------------------------------------------------------
// Ops gives n (the elements), z (where the preconditioned residual lands) and three steps, each RSM_OK or an error once its sum is on the host:
//   precondition(&rho)   z = M^-1 r and rho = r . z
//   apply(p, q, &pq)     q = A p and pq = p . q
//   residual(chi, &rr)   r = b - A chi and rr = r . r
// On entry r belongs to d_chi, *residual is its norm over bnorm = |b|, above rel_residual, and `best` holds d_chi.  The residual is recomputed
// from chi, not updated by recurrence: what is reported is what chi reaches.  Float32 conjugate gradients reach a floor (a few 1e-6) and drift
// away from it afterwards: the best chi is kept, `stall` iterations in a row without a new best end the solve, and d_chi leaves as the best
// iterate.  history (optional): the residual after each iteration.  Enqueues and waits for the sums; the caller waits for the end.
template <class Ops>
static int poisson_pcg(Ops &A, double bnorm, double rel_residual, int max_iterations, int stall, float *d_chi, float *p, float *q, float *best, double *residual,
                       int *iterations, double *history, hipStream_t st) {
    const size_t n = A.n;
    double rho_old = 0.0;
    int worse = 0, s;
    for (int it = 1; it <= max_iterations; it++) {
        double rho = 0.0, pq = 0.0, rr = 0.0;
        if ((s = A.precondition(&rho)) != RSM_OK) return s;
        if (it == 1) DEVCHK(hipMemcpyAsync(p, A.z, n * sizeof(float), hipMemcpyDeviceToDevice, st));
        else hipLaunchKernelGGL(k_pv_xpay<>, blocks_for(n), dim3(256), 0, st, p, (const float *)A.z, (float)(rho / rho_old), n);
        if ((s = A.apply(p, q, &pq)) != RSM_OK) return s;
        if (pq == 0.0 || !std::isfinite(rho / pq)) break; // nothing left to correct in float32
        hipLaunchKernelGGL(k_pv_axpy<>, blocks_for(n), dim3(256), 0, st, d_chi, (const float *)p, (float)(rho / pq), n);
        if ((s = A.residual(d_chi, &rr)) != RSM_OK) return s;
        rho_old = rho;
        *iterations = it;
        const double res = sqrt(rr) / bnorm;
        if (history) history[it - 1] = res;
        if (res < *residual) {
            *residual = res;
            worse = 0;
            if (res <= rel_residual) break; // (chi is the best iterate)
            DEVCHK(hipMemcpyAsync(best, d_chi, n * sizeof(float), hipMemcpyDeviceToDevice, st));
        } else if (++worse >= stall)
            break;
    }
    if (*residual > rel_residual) DEVCHK(hipMemcpyAsync(d_chi, best, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return RSM_OK;
}

// ---- host: the iso-value = the mean of chi at the n samples.  launch_chi(val) enqueues chi at the samples; d_w (optional): their weights, the
// mean is sum w chi / denominator (f14's product and f7's tree), else sum chi / denominator.  denominator <= 0: 0 -----------------------------------
template <class LaunchChi>
static int poisson_mean_of_chi_at_samples(LaunchChi launch_chi, int64_t n, const double *d_w, double denominator, double *mean, hipStream_t st) {
    *mean = 0.0;
    if (n <= 0 || !(denominator > 0.0)) return RSM_OK;
    DevMem M;
    double *val = M.get<double>((size_t)n), *part = d_w ? nullptr : M.get<double>(POISSON_SUM_PARTIALS), *scal = d_w ? nullptr : M.get<double>(1);
    if (!M.ok) return RSM_E_NOMEM;
    launch_chi(val);
    if (d_w) return poisson_weighted_mean_device(val, d_w, n, denominator, mean, st);
    poisson_tree_sum(val, n, part, scal, st);
    double sum = 0.0;
    DEVCHK(hipMemcpyAsync(&sum, scal, sizeof sum, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    *mean = sum / denominator;
    return RSM_OK;
}
