// k_meshtrim.hip -- the density trim of the Poisson surface, where mesh.bat runs PoissonRecon --density and then SurfaceTrimmer --smooth 100
// --trim 7 --aRatio 0.01.  Not a bit-parity port of those tools (no source in the reference tree): every rule is defined in
// DESIGN.md 9 (f11) and restated in numpy in tests/meshtrim_restatement.py, and the kernels are held to that restatement exactly.
//   count splat   C(node) += llrint(w 2^32) over the 8 nodes of f7's trilinear weights on the coarser grid of 2^kernel_depth nodes per axis,
//                 64-bit integer atomics: no order in the sum.  w <= 1 and a sample meets a node once, so INT32_MAX samples stay below
//                 (2^31 - 1) 2^32 < 2^63                                                                             k_mt_splat
//   value         rho = the same weights times C 2^-32, eight fp64 terms in the corner order dz, dy, dx; value = max(0, kernel_depth +
//                 1/2 log2(rho / samples_per_node))                                                                  k_mt_value
//   smoothing     neighbour CSR in the order of mesh_common.h's corner lists (as k_mst_csr), one gather launch per step, values ping-pong, no host
//                 synchronisation inside the loop                                                                   k_mesh_nbr_csr, k_mt_step
//   split         the first entry of a run of mesh_common.h's sorted edge table whose ends lie on different sides of `trim` is a cut edge; its rank
//                 among them (a scan) numbers its vertex; faces count 0 / 1 / 3 triangles, scan, emit               k_mt_cut_flags .. k_mt_face_emit
//   islands       the edge table of the split mesh, union-find per side, areas as 64-bit fixed point (llrint(area 2^32 / D^2) <= 2^31 per
//                 triangle and fewer than 2^31 triangles: every sum stays below 2^62), integer atomics behind a per-block reduction for the
//                 one giant component                                                                               k_mt_unite, k_mt_areas, k_mt_decide
//   compaction    the kept triangles and the vertices they use, renumbered in order (dev_prims.h)
// The count splat and the value are also what the density-adaptive Poisson splat weighs its samples by (k_poisson_density.hip; DESIGN.md 9
// f14): it calls density_at_points_device below with the samples themselves as the points.
// No float atomics.  Built with -ffp-contract=off (csrc/Makefile): every fp64 expression below is evaluated as written.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"

#include <string.h>

#include <math.h>

#include <algorithm>

#define MT_FIX 4294967296.0 // 2^32: the fixed-point scale of the counts and the areas

namespace {

typedef unsigned long long u64;

enum { T_CUT = 0, T_SPLIT, T_REPEAT, T_ZERO, T_COMP_KEPT, T_COMP_DROPPED, T_MOVED_KD, T_MOVED_DK, T_QTOTAL, T_VMIN, T_VMAX, T_N };

__device__ __forceinline__ void count_if(bool flag, u64 *ctr) {
    if (flag) atomicAdd(ctr, (u64)1);
}

// ---- 2: the count splat ---------------------------------------------------------------------------------------------------------------
// (mesh_common.h: MtGrid, mt_cell, mt_weight -- f7's trilinear cell and weights, shared with k_poisson_density.hip)
template <bool HAS_N>
__global__ __launch_bounds__(256) void k_mt_splat(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t n, MtGrid g, u64 *__restrict__ C) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    double p[3], nh[3], fl[3], f[3];
    if (!(HAS_N ? pv_valid(xyz, nrm, s, p, nh) : pv_valid_point(xyz, s, p))) return;
    mt_cell(p, g, fl, f);
    const int N = g.N;
    // (a valid sample lies inside the box, so fl is in [-1, N - 1]; the test keeps a cast of anything else out)
    if (!(fl[0] >= -1.0 && fl[1] >= -1.0 && fl[2] >= -1.0 && fl[0] < (double)N && fl[1] < (double)N && fl[2] < (double)N)) return;
    const int i0[3] = {(int)fl[0], (int)fl[1], (int)fl[2]};
    for (int dz = 0; dz < 2; dz++)
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const int i = i0[0] + dx, j = i0[1] + dy, k = i0[2] + dz;
                if (i < 0 || j < 0 || k < 0 || i >= N || j >= N || k >= N) continue;
                const long long q = __double2ll_rn(mt_weight(f, dx, dy, dz) * MT_FIX);
                if (q) atomicAdd(&C[(size_t)i + (size_t)N * ((size_t)j + (size_t)N * k)], (u64)q);
            }
}

// ---- 3: the density and the value at the vertices -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mt_value(const float *__restrict__ v, size_t nv, MtGrid g, const long long *__restrict__ C, double kd, double spn,
                                                  double *__restrict__ rho, double *__restrict__ val) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nv) return;
    const double p[3] = {(double)v[3 * t], (double)v[3 * t + 1], (double)v[3 * t + 2]};
    double fl[3], f[3], acc = 0.0;
    mt_cell(p, g, fl, f);
    const int N = g.N;
    if (fl[0] >= -1.0 && fl[1] >= -1.0 && fl[2] >= -1.0 && fl[0] < (double)N && fl[1] < (double)N && fl[2] < (double)N) {
        const int i0[3] = {(int)fl[0], (int)fl[1], (int)fl[2]};
        for (int dz = 0; dz < 2; dz++)
            for (int dy = 0; dy < 2; dy++)
                for (int dx = 0; dx < 2; dx++) {
                    const int i = i0[0] + dx, j = i0[1] + dy, k = i0[2] + dz;
                    if (i < 0 || j < 0 || k < 0 || i >= N || j >= N || k >= N) continue;
                    const double c = (double)C[(size_t)i + (size_t)N * ((size_t)j + (size_t)N * k)] / MT_FIX;
                    acc += mt_weight(f, dx, dy, dz) * c;
                }
    }
    double x = 0.0;
    if (acc > 0.0) {
        x = kd + 0.5 * log2(acc / spn);
        x = x > 0.0 ? x : 0.0;
    }
    if (rho) rho[t] = acc;
    val[t] = x;
}

// ---- 4: smoothing of the values ---------------------------------------------------------------------------------------------------------
// the neighbour CSR is mesh_common.h's (k_mesh_nbr_csr): row i starts at 2 row[i] and holds deg[i] = 2 (row[i + 1] - row[i]) entries
__global__ __launch_bounds__(256) void k_mt_step(const double *__restrict__ in, double *__restrict__ out, size_t nv, const uint32_t *__restrict__ row,
                                                 const uint32_t *__restrict__ nbr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const size_t b = 2 * (size_t)row[i], e = 2 * (size_t)row[i + 1];
    const double x = in[i];
    if (b == e) { // an unreferenced vertex keeps its value
        out[i] = x;
        return;
    }
    double s = 0.0;
    for (size_t t = b; t < e; t++) s += in[nbr[t]];
    out[i] = (x + s) / (1.0 + (double)(e - b));
}

// the order-preserving map double -> u64 (integer atomicMin / atomicMax on it give the exact min / max) and back
__host__ __device__ __forceinline__ u64 d2ord(double d) {
    u64 u;
    __builtin_memcpy(&u, &d, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
static double ord2d(u64 u) {
    const u64 v = (u >> 63) ? (u ^ 0x8000000000000000ull) : ~u;
    double d;
    memcpy(&d, &v, 8);
    return d;
}
__global__ __launch_bounds__(256) void k_mt_minmax(const double *__restrict__ x, size_t nv, u64 *__restrict__ ctr) {
    __shared__ u64 s_mm[2];
    if (threadIdx.x == 0) {
        s_mm[0] = ~0ull;
        s_mm[1] = 0ull;
    }
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const u64 o = d2ord(x[i]);
        atomicMin(&s_mm[0], o);
        atomicMax(&s_mm[1], o);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(ctr + T_VMIN, s_mm[0]);
        atomicMax(ctr + T_VMAX, s_mm[1]);
    }
}

// ---- 5: the split -----------------------------------------------------------------------------------------------------------------------
// flag[i] = sorted entry i is the first of its run and its edge is cut
__global__ __launch_bounds__(256) void k_mt_cut_flags(const u64 *__restrict__ key, size_t n, u64 nv, const double *__restrict__ x, double trim,
                                                      unsigned int *__restrict__ flag, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool cut = false;
    if (i < n) {
        const u64 k = key[i];
        if ((k >> 32) != nv && !(i > 0 && key[i - 1] == k)) cut = (x[k >> 32] >= trim) != (x[k & 0xffffffffu] >= trim);
        flag[i] = cut ? 1u : 0u;
    }
    count_if(cut, ctr + T_CUT);
}
// the cut vertex of edge (lo, hi) at nv + its rank
__global__ __launch_bounds__(256) void k_mt_cut_verts(const u64 *__restrict__ key, size_t n, const unsigned int *__restrict__ flag,
                                                      const unsigned int *__restrict__ pos, const double *__restrict__ x, double trim, size_t nv,
                                                      float *__restrict__ sv) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const size_t lo = (size_t)(key[i] >> 32), hi = (size_t)(key[i] & 0xffffffffu);
    const double t = (trim - x[lo]) / (x[hi] - x[lo]);
    const size_t o = nv + pos[i];
    for (int a = 0; a < 3; a++) {
        const double pl = (double)sv[3 * lo + a], ph = (double)sv[3 * hi + a];
        sv[3 * o + a] = (float)(pl + t * (ph - pl));
    }
}
// ecut[3 f + j] = the cut vertex of face f's edge j, -1 (the array's fill) when the edge is not cut
__global__ __launch_bounds__(256) void k_mt_edge_cut(const u64 *__restrict__ key, const uint32_t *__restrict__ val, size_t n, u64 nv,
                                                     const unsigned int *__restrict__ flag, const unsigned int *__restrict__ pos, int32_t *__restrict__ ecut) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    if ((k >> 32) == nv) return;
    size_t q = i;
    while (q > 0 && key[q - 1] == k) q--;
    if (flag[q]) ecut[val[i]] = (int32_t)(nv + pos[q]);
}
// triangles a face becomes: 0 (a repeated index), 1 (its corners on one side) or 3
__global__ __launch_bounds__(256) void k_mt_face_count(const int32_t *__restrict__ f, size_t nf, const double *__restrict__ x, double trim,
                                                       unsigned int *__restrict__ cnt, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool rep = false, spl = false;
    if (i < nf) {
        const int a = f[3 * i], b = f[3 * i + 1], c = f[3 * i + 2];
        rep = !face_distinct(a, b, c);
        if (!rep) {
            const bool ka = x[a] >= trim, kb = x[b] >= trim, kc = x[c] >= trim;
            spl = !(ka == kb && kb == kc);
        }
        cnt[i] = rep ? 0u : (spl ? 3u : 1u);
    }
    count_if(rep, ctr + T_REPEAT);
    count_if(spl, ctr + T_SPLIT);
}

__device__ __forceinline__ double dist2(const D3 &a, const D3 &b) {
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}
// |(P1 - P0) x (P2 - P0)|^2, in the project's order (a0 b0 + a1 b1) + a2 b2
__device__ __forceinline__ double tri_n2(const D3 &p0, const D3 &p1, const D3 &p2) {
    const double u0 = p1.x - p0.x, u1 = p1.y - p0.y, u2 = p1.z - p0.z;
    const double w0 = p2.x - p0.x, w1 = p2.y - p0.y, w2 = p2.z - p0.z;
    const double c0 = u1 * w2 - u2 * w1, c1 = u2 * w0 - u0 * w2, c2 = u0 * w1 - u1 * w0;
    return (c0 * c0 + c1 * c1) + c2 * c2;
}

__global__ __launch_bounds__(256) void k_mt_face_emit(const int32_t *__restrict__ f, size_t nf, const double *__restrict__ x, double trim,
                                                      const unsigned int *__restrict__ cnt, const unsigned int *__restrict__ off, const int32_t *__restrict__ ecut,
                                                      const float *__restrict__ sv, int32_t *__restrict__ tri, int32_t *__restrict__ tsrc,
                                                      uint8_t *__restrict__ tside, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    u64 zero = 0;
    if (i < nf && cnt[i]) {
        const int v[3] = {f[3 * i], f[3 * i + 1], f[3 * i + 2]};
        const bool k[3] = {x[v[0]] >= trim, x[v[1]] >= trim, x[v[2]] >= trim};
        const size_t o = off[i];
        if (cnt[i] == 1) {
            for (int c = 0; c < 3; c++) tri[3 * o + c] = v[c];
            tsrc[o] = (int32_t)i;
            tside[o] = k[0];
        } else {
            const int j = (k[0] != k[1] && k[0] != k[2]) ? 0 : (k[1] != k[0] ? 1 : 2); // the corner alone on its side
            const int a = v[j], b = v[(j + 1) % 3], c = v[(j + 2) % 3];
            const int ab = ecut[3 * i + j], ca = ecut[3 * i + (j + 2) % 3];
            if (ab < 0 || ca < 0) { // (never: both edges at `a` are cut by k_mt_cut_flags' own test; the slots still get indices that can be read)
                for (int m = 0; m < 3; m++) {
                    for (int e = 0; e < 3; e++) tri[3 * (o + m) + e] = a;
                    tsrc[o + m] = (int32_t)i;
                    tside[o + m] = 0;
                }
            } else {
                const D3 q0 = ld3(sv, ab), q1 = ld3(sv, b), q2 = ld3(sv, c), q3 = ld3(sv, ca);
                const bool d13 = dist2(q1, q3) < dist2(q0, q2);
                const int t[3][3] = {{a, ab, ca}, {ab, b, d13 ? ca : c}, {d13 ? b : ab, c, ca}};
                for (int m = 0; m < 3; m++) {
                    for (int e = 0; e < 3; e++) tri[3 * (o + m) + e] = t[m][e];
                    tsrc[o + m] = (int32_t)i;
                    tside[o + m] = m == 0 ? k[j] : k[(j + 1) % 3];
                    zero += tri_n2(ld3(sv, t[m][0]), ld3(sv, t[m][1]), ld3(sv, t[m][2])) == 0.0;
                }
            }
        }
    }
    if (zero) atomicAdd(ctr + T_ZERO, zero);
}

// ---- 6: islands ---------------------------------------------------------------------------------------------------------------------------
// one thread per sorted entry of the split mesh's edge table: its triangle joins the nearest earlier one of the run that lies on its side
__global__ __launch_bounds__(256) void k_mt_unite(const u64 *__restrict__ key, const uint32_t *__restrict__ val, size_t n, u64 nv, const uint8_t *__restrict__ tside,
                                                  int *__restrict__ parent) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    if ((k >> 32) == nv) return;
    const int t = (int)(val[i] / 3);
    for (size_t q = i; q > 0 && key[q - 1] == k; q--) {
        const int u = (int)(val[q - 1] / 3);
        if (tside[u] == tside[t]) {
            uf_union(parent, t, u);
            return;
        }
    }
}
// (runs after every union, in a launch of its own)
__global__ __launch_bounds__(256) void k_mt_labels(int *__restrict__ parent, size_t nt, int32_t *__restrict__ label) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nt) label[i] = uf_find(parent, (int)i);
}
// Q[label] += q, the total, and touch[label] = the component holds a triangle of a split face.  One giant component is the contention case:
// the threads of a block that share thread 0's label add up in LDS first, one atomic per block
__global__ __launch_bounds__(256) void k_mt_areas(const float *__restrict__ sv, const int32_t *__restrict__ tri, size_t nt, const int32_t *__restrict__ label,
                                                  const int32_t *__restrict__ tsrc, const unsigned int *__restrict__ fcnt, const unsigned int *__restrict__ box,
                                                  u64 *__restrict__ Q, uint8_t *__restrict__ touch, u64 *__restrict__ ctr) {
    __shared__ u64 s_q, s_tot;
    __shared__ int s_lab;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lab = i < nt ? label[i] : -1;
    if (threadIdx.x == 0) {
        s_lab = lab;
        s_q = s_tot = 0;
    }
    __syncthreads();
    if (lab >= 0) {
        const double D2 = box_diagonal2(box);
        long long q = 0;
        if (D2 > 0.0) {
            const double area = 0.5 * sqrt(tri_n2(ld3(sv, tri[3 * i]), ld3(sv, tri[3 * i + 1]), ld3(sv, tri[3 * i + 2])));
            q = __double2ll_rn((area * MT_FIX) / D2);
        }
        if (fcnt[tsrc[i]] == 3u) touch[lab] = 1; // (every writer stores the same value)
        if (q > 0) {
            atomicAdd(&s_tot, (u64)q);
            if (lab == s_lab) atomicAdd(&s_q, (u64)q);
            else atomicAdd(Q + lab, (u64)q);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_q) atomicAdd(Q + s_lab, s_q);
        if (s_tot) atomicAdd(ctr + T_QTOTAL, s_tot);
    }
}
__global__ __launch_bounds__(256) void k_mt_decide(const int32_t *__restrict__ tri, size_t nt, const int32_t *__restrict__ label, const uint8_t *__restrict__ tside,
                                                   const u64 *__restrict__ Q, const uint8_t *__restrict__ touch, double ratio, unsigned int *__restrict__ fkeep,
                                                   unsigned int *__restrict__ vused, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool root_k = false, root_d = false, mv_k = false, mv_d = false;
    if (i < nt) {
        const int lab = label[i];
        const u64 total = ctr[T_QTOTAL]; // (written by the launch before)
        const bool moves = ratio > 0.0 && total > 0 && touch[lab] && (double)Q[lab] < ratio * (double)total;
        const bool side = tside[i] != 0;
        const bool keep = side != moves;
        fkeep[i] = keep ? 1u : 0u;
        if (keep) vused[tri[3 * i]] = vused[tri[3 * i + 1]] = vused[tri[3 * i + 2]] = 1u; // (every writer stores the same value)
        if (lab == (int)i) {
            root_k = side;
            root_d = !side;
            mv_k = moves && side;
            mv_d = moves && !side;
        }
    }
    count_if(root_k, ctr + T_COMP_KEPT);
    count_if(root_d, ctr + T_COMP_DROPPED);
    count_if(mv_k, ctr + T_MOVED_KD);
    count_if(mv_d, ctr + T_MOVED_DK);
}
// per output face its source face, its side before the island rule and its label
__global__ __launch_bounds__(256) void k_mt_compact_info(size_t nt, const unsigned int *__restrict__ fkeep, const unsigned int *__restrict__ fpos,
                                                         const int32_t *__restrict__ tsrc, const uint8_t *__restrict__ tside, const int32_t *__restrict__ label,
                                                         int32_t *__restrict__ osrc, int32_t *__restrict__ oside, int32_t *__restrict__ olabel) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt || !fkeep[i]) return;
    const size_t o = fpos[i];
    if (osrc) osrc[o] = tsrc[i];
    if (oside) oside[o] = tside[i];
    if (olabel) olabel[o] = label[i];
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
static dim3 red_grid(size_t n) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>(1024, (n + 255) / 256))); }

// rules 2 and 3 on a box that is known (grid = f7's {o, h}, hk = side / 2^kd > 0): the count splat of the samples, read back at nv > 0 points.
// Enqueues only; the counts are M's and live as long as M
static int density_on_grid(DevMem &M, const float *d_sx, const float *d_sn4, int64_t n, const double grid[4], double hk, int kd, double spn, const float *d_v,
                           size_t nv, double *d_rho, double *d_val, hipStream_t st) {
    const size_t N3 = (size_t)1 << (3 * kd);
    u64 *C = M.get<u64>(N3);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(C, 0, N3 * sizeof(u64), st));
    const MtGrid g{grid[0], grid[1], grid[2], hk, 1 << kd};
    if (d_sn4) hipLaunchKernelGGL(k_mt_splat<true>, blocks_for((size_t)n), dim3(256), 0, st, d_sx, d_sn4, n, g, C);
    else hipLaunchKernelGGL(k_mt_splat<false>, blocks_for((size_t)n), dim3(256), 0, st, d_sx, d_sn4, n, g, C);
    hipLaunchKernelGGL(k_mt_value, blocks_for(nv), dim3(256), 0, st, d_v, nv, g, (const long long *)C, (double)kd, spn, d_rho, d_val);
    return RSM_OK;
}

// rho (optional) and value at nv > 0 vertices; *hk = 0: no valid sample or all of them equal, every value 0
static int density(DevMem &M, const float *d_sx, const float *d_sn4, int64_t n, int depth, double scale, int kd, double spn, const float *d_v, size_t nv,
                   double *d_rho, double *d_val, int64_t counts[2], double *hk, hipStream_t st) {
    double grid[4];
    int s = poisson_grid_device(d_sx, d_sn4, n, depth, scale, grid, counts, st);
    if (s != RSM_OK) return s;
    *hk = grid[3] * (double)(1 << (depth - kd)); // side / 2^kd: h = side / 2^depth, and the powers of two are exact
    if (nv == 0) return RSM_OK;
    if (!(*hk > 0.0)) {
        if (d_rho) DEVCHK(hipMemsetAsync(d_rho, 0, nv * sizeof(double), st));
        DEVCHK(hipMemsetAsync(d_val, 0, nv * sizeof(double), st));
        return RSM_OK;
    }
    return density_on_grid(M, d_sx, d_sn4, n, grid, *hk, kd, spn, d_v, nv, d_rho, d_val, st);
}

// `steps` steps from d_in (nv > 0 values); the result is in *d_res (d_in itself with steps = 0 or no face, else one of two scratch buffers)
static int smooth_values(DevMem &M, const int32_t *d_f, size_t nv, size_t nf, const double *d_in, int steps, const double **d_res, hipStream_t st) {
    *d_res = d_in;
    if (steps <= 0 || nf == 0) return RSM_OK;
    uint32_t *corner = nullptr, *row = nullptr;
    const int s = mesh_corner_lists(M, d_f, nv, nf, &row, &corner, st);
    if (s != RSM_OK) return s;
    uint32_t *nbr = M.get<uint32_t>(6 * nf);
    double *buf[2] = {M.get<double>(nv), M.get<double>(nv)};
    if (!M.ok) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_mesh_nbr_csr<>, blocks_for(nv), dim3(256), 0, st, nv, d_f, (const uint32_t *)row, (const uint32_t *)corner, nbr);
    const double *src = d_in;
    for (int it = 0; it < steps; it++) {
        double *dst = buf[it & 1];
        hipLaunchKernelGGL(k_mt_step, blocks_for(nv), dim3(256), 0, st, src, dst, nv, (const uint32_t *)row, (const uint32_t *)nbr);
        src = dst;
    }
    *d_res = src;
    return RSM_OK;
}

// rules 5-7 on a validated mesh and nv values.  S: RSM_MESH_TRIM_STATS doubles, filled from [0..3] and [6] on
static int split(DevMem &M, const float *d_v, size_t nv, const int32_t *d_f, size_t nf, const double *d_x, double trim, double ratio, PoissonMesh *out,
                 int32_t *d_src, int32_t *d_side, int32_t *d_label, double *S, hipStream_t st) {
    PoissonMesh res;
    S[0] = (double)nv;
    S[1] = (double)nf;
    u64 h[T_N] = {0};
    unsigned int hbox[6] = {0, 0, 0, 0, 0, 0};
    if (nv > 0 && nf > 0) {
        const size_t n = 3 * nf;
        u64 *ctr = M.get<u64>(T_N);
        unsigned int *box = M.get<unsigned int>(6);
        u64 *k0 = M.get<u64>(n), *ekey = M.get<u64>(n);
        uint32_t *v0 = M.get<uint32_t>(n), *eval = M.get<uint32_t>(n);
        unsigned int *cflag = M.get<unsigned int>(n), *cpos = M.get<unsigned int>(n), *fcnt = M.get<unsigned int>(nf), *foff = M.get<unsigned int>(nf);
        int32_t *ecut = M.get<int32_t>(n);
        if (!M.ok) return RSM_E_NOMEM;
        const u64 init[T_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0, ~0ull, 0};
        const unsigned int binit[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
        DEVCHK(hipMemcpyAsync(ctr, init, sizeof init, hipMemcpyHostToDevice, st));
        DEVCHK(hipMemcpyAsync(box, binit, sizeof binit, hipMemcpyHostToDevice, st));
        DEVCHK(hipMemsetAsync(ecut, 0xff, n * sizeof(int32_t), st));
        hipLaunchKernelGGL(k_mesh_vertex_box<>, red_grid(nv), dim3(256), 0, st, d_v, nv, box);
        hipLaunchKernelGGL(k_mt_minmax, red_grid(nv), dim3(256), 0, st, d_x, nv, ctr);
        // the input's edge table, the cut edges ranked
        int s = mesh_edge_table(M, d_f, nv, nf, k0, v0, ekey, eval, st);
        if (s != RSM_OK) return s;
        hipLaunchKernelGGL(k_mt_cut_flags, blocks_for(n), dim3(256), 0, st, (const u64 *)ekey, n, (u64)nv, d_x, trim, cflag, ctr);
        hipLaunchKernelGGL(k_mt_face_count, blocks_for(nf), dim3(256), 0, st, d_f, nf, d_x, trim, fcnt, ctr);
        if ((s = scan_u32(M, (const unsigned int *)cflag, cpos, n, st)) != RSM_OK || (s = scan_u32(M, (const unsigned int *)fcnt, foff, nf, st)) != RSM_OK) return s;
        uint64_t ncut = 0, nt = 0;
        if ((s = scan_totals(cflag, cpos, n, fcnt, foff, nf, st, &ncut, &nt)) != RSM_OK) return s;
        if (3 * nt > (uint64_t)UINT32_MAX) return RSM_E_NOMEM; // (an edge table entry is a uint32; 1.4e9 triangles do not fit the device either)
        if (nt > 0) {
            const size_t nvs = nv + (size_t)ncut, m = 3 * (size_t)nt;
            float *sv = M.get<float>(3 * nvs);
            int32_t *tri = M.get<int32_t>(m), *tsrc = M.get<int32_t>(nt), *label = M.get<int32_t>(nt);
            uint8_t *tside = M.get<uint8_t>(nt), *touch = M.get<uint8_t>(nt);
            u64 *sk0 = M.get<u64>(m), *skey = M.get<u64>(m), *Q = M.get<u64>(nt);
            uint32_t *sv0 = M.get<uint32_t>(m), *sval = M.get<uint32_t>(m);
            int *parent = M.get<int>(nt);
            unsigned int *fkeep = M.get<unsigned int>(nt), *fpos = M.get<unsigned int>(nt), *vused = M.get<unsigned int>(nvs), *vpos = M.get<unsigned int>(nvs);
            if (!M.ok) return RSM_E_NOMEM;
            DEVCHK(hipMemcpyAsync(sv, d_v, 3 * nv * sizeof(float), hipMemcpyDeviceToDevice, st));
            DEVCHK(hipMemsetAsync(touch, 0, nt, st));
            DEVCHK(hipMemsetAsync(Q, 0, nt * sizeof(u64), st));
            DEVCHK(hipMemsetAsync(vused, 0, nvs * sizeof(unsigned int), st));
            hipLaunchKernelGGL(k_mt_cut_verts, blocks_for(n), dim3(256), 0, st, (const u64 *)ekey, n, (const unsigned int *)cflag, (const unsigned int *)cpos, d_x, trim,
                               nv, sv);
            hipLaunchKernelGGL(k_mt_edge_cut, blocks_for(n), dim3(256), 0, st, (const u64 *)ekey, (const uint32_t *)eval, n, (u64)nv, (const unsigned int *)cflag,
                               (const unsigned int *)cpos, ecut);
            hipLaunchKernelGGL(k_mt_face_emit, blocks_for(nf), dim3(256), 0, st, d_f, nf, d_x, trim, (const unsigned int *)fcnt, (const unsigned int *)foff,
                               (const int32_t *)ecut, (const float *)sv, tri, tsrc, tside, ctr);
            // the split mesh's edge table, components per side, areas, the island rule
            if ((s = mesh_edge_table(M, (const int32_t *)tri, nvs, (size_t)nt, sk0, sv0, skey, sval, st)) != RSM_OK) return s;
            hipLaunchKernelGGL(k_mesh_iota<>, blocks_for(nt), dim3(256), 0, st, parent, (size_t)nt);
            hipLaunchKernelGGL(k_mt_unite, blocks_for(m), dim3(256), 0, st, (const u64 *)skey, (const uint32_t *)sval, m, (u64)nvs, (const uint8_t *)tside, parent);
            hipLaunchKernelGGL(k_mt_labels, blocks_for(nt), dim3(256), 0, st, parent, (size_t)nt, label);
            hipLaunchKernelGGL(k_mt_areas, blocks_for(nt), dim3(256), 0, st, (const float *)sv, (const int32_t *)tri, (size_t)nt, (const int32_t *)label,
                               (const int32_t *)tsrc, (const unsigned int *)fcnt, (const unsigned int *)box, Q, touch, ctr);
            hipLaunchKernelGGL(k_mt_decide, blocks_for(nt), dim3(256), 0, st, (const int32_t *)tri, (size_t)nt, (const int32_t *)label, (const uint8_t *)tside,
                               (const u64 *)Q, (const uint8_t *)touch, ratio, fkeep, vused, ctr);
            if ((s = scan_u32(M, (const unsigned int *)fkeep, fpos, nt, st)) != RSM_OK || (s = scan_u32(M, (const unsigned int *)vused, vpos, nvs, st)) != RSM_OK) return s;
            uint64_t kf = 0, kv = 0;
            if ((s = scan_totals(fkeep, fpos, nt, vused, vpos, nvs, st, &kf, &kv)) != RSM_OK) return s;
            if (kf > 0) {
                if ((s = mesh_result_alloc(res, kv, kf)) != RSM_OK) return s;
                hipLaunchKernelGGL(k_mesh_compact_faces<>, blocks_for(nt), dim3(256), 0, st, (const int32_t *)tri, (size_t)nt, (const unsigned int *)fkeep,
                                   (const unsigned int *)fpos, (const unsigned int *)vpos, res.d_f);
                hipLaunchKernelGGL(k_mesh_compact_verts<>, blocks_for(nvs), dim3(256), 0, st, (const float *)sv, nvs, (const unsigned int *)vused,
                                   (const unsigned int *)vpos, res.d_v);
                if (d_src || d_side || d_label)
                    hipLaunchKernelGGL(k_mt_compact_info, blocks_for(nt), dim3(256), 0, st, (size_t)nt, (const unsigned int *)fkeep, (const unsigned int *)fpos,
                                       (const int32_t *)tsrc, (const uint8_t *)tside, (const int32_t *)label, d_src, d_side, d_label);
            }
        }
        if (hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess || hipMemcpyAsync(hbox, box, sizeof hbox, hipMemcpyDeviceToHost, st) != hipSuccess ||
            mesh_finish(st) != RSM_OK) {
            poisson_mesh_free(&res);
            return RSM_E_HIP;
        }
        S[15] = ord2d(h[T_VMIN]);
        S[16] = ord2d(h[T_VMAX]);
        S[17] = box_diagonal2(hbox);
    }
    S[2] = (double)res.nv;
    S[3] = (double)res.nf;
    S[6] = (double)h[T_CUT];
    S[7] = (double)h[T_SPLIT];
    S[8] = (double)h[T_REPEAT];
    S[9] = (double)h[T_ZERO];
    S[10] = (double)h[T_COMP_KEPT];
    S[11] = (double)h[T_COMP_DROPPED];
    S[12] = (double)h[T_MOVED_KD];
    S[13] = (double)h[T_MOVED_DK];
    S[14] = (double)h[T_QTOTAL];
    mesh_result_commit(out, res);
    return RSM_OK;
}

} // namespace

int mesh_density_device(const float *d_sx, const float *d_sn4, int64_t n, int depth, double scale, int kernel_depth, double samples_per_node, const float *d_v,
                        int64_t nv, double *d_rho, double *d_val, int64_t counts[2], double *hk, int *invalid, hipStream_t st) {
    DevMem M;
    int s = mesh_validate_device(d_v, nv, nullptr, 0, invalid, st);
    if (s != RSM_OK) return s;
    s = density(M, d_sx, d_sn4, n, depth, scale, kernel_depth, samples_per_node, d_v, (size_t)nv, d_rho, d_val, counts, hk, st);
    return s != RSM_OK ? s : mesh_finish(st);
}

int density_at_points_device(DevMem &M, const float *d_sx, const float *d_sn4, int64_t n, int depth, const double grid[4], int kernel_depth,
                             double samples_per_node, const float *d_v, int64_t nv, double *d_rho, double *d_val, hipStream_t st) {
    if (nv <= 0) return RSM_OK;
    return density_on_grid(M, d_sx, d_sn4, n, grid, grid[3] * (double)(1 << (depth - kernel_depth)), kernel_depth, samples_per_node, d_v, (size_t)nv, d_rho, d_val,
                           st);
}

int mesh_value_smooth_device(const int32_t *d_f, int64_t nv, int64_t nf, const double *d_in, int steps, double *d_out, int *invalid, hipStream_t st) {
    int s = mesh_validate_device(nullptr, nv, d_f, nf, invalid, st);
    if (s != RSM_OK || nv <= 0) return s;
    DevMem M;
    const double *res = d_in;
    s = smooth_values(M, d_f, (size_t)nv, (size_t)nf, d_in, steps, &res, st);
    if (s != RSM_OK) return s;
    DEVCHK(hipMemcpyAsync(d_out, res, (size_t)nv * sizeof(double), hipMemcpyDeviceToDevice, st));
    return mesh_finish(st);
}

int mesh_split_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const double *d_val, double trim, double island_ratio, PoissonMesh *out,
                      int32_t *d_src, int32_t *d_side, int32_t *d_label, double *stats, int *invalid, hipStream_t st) {
    DevMem M;
    double S[RSM_MESH_TRIM_STATS] = {0};
    int s = mesh_validate_device(d_v, nv, d_f, nf, invalid, st);
    if (s != RSM_OK) return s;
    s = split(M, d_v, (size_t)nv, d_f, (size_t)nf, d_val, trim, island_ratio, out, d_src, d_side, d_label, S, st);
    if (s == RSM_OK && stats) memcpy(stats, S, sizeof S);
    return s;
}

int mesh_trim_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const float *d_sx, const float *d_sn4, int64_t n, const rsm_mesh_trim_params *p,
                     PoissonMesh *out, double *stats, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    double S[RSM_MESH_TRIM_STATS] = {0};
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK) return s;
    const int kd = p->kernel_depth ? p->kernel_depth : p->depth - 2;
    DevMem M;
    int64_t counts[2] = {0, n};
    double hk = 0.0;
    double *val = M.get<double>(nv);
    if (!M.ok) return RSM_E_NOMEM;
    const double *x = val;
    if ((s = density(M, d_sx, d_sn4, n, p->depth, p->scale, kd, p->samples_per_node, d_v, nv, nullptr, val, counts, &hk, st)) != RSM_OK) return s;
    if (nv > 0 && (s = smooth_values(M, d_f, nv, nf, val, p->smooth_steps, &x, st)) != RSM_OK) return s;
    if ((s = split(M, d_v, nv, d_f, nf, x, p->trim, p->island_ratio, out, nullptr, nullptr, nullptr, S, st)) != RSM_OK) return s;
    S[4] = (double)counts[0];
    S[5] = (double)counts[1];
    S[18] = hk;
    S[19] = (double)kd;
    if (stats) memcpy(stats, S, sizeof S);
    return RSM_OK;
}
