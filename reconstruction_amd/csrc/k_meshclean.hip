// k_meshclean.hip -- what meshlab.bat does to the Poisson surface after reconstructing it: script1.mlx's
// "Laplacian Smooth" (5 steps, cotangent weighting, 1D boundary smoothing) and script2.mlx's "Remove Isolated pieces (wrt Diameter)",
// "Remove Duplicate Faces", "Remove Zero Area Faces" and "Remove Faces from Non Manifold Edges", in that order.  Not a bit-parity port of
// MeshLab / VCG (no source in the reference tree): every rule is defined in DESIGN.md 9 (f8) and restated in numpy in
// tests/meshclean_restatement.py, and the kernels are held to that restatement exactly.
//   edge table    mesh_common.h's sorted table (mesh_edge_table); a run of equal keys = the faces on one edge (its incidence)      k_mc_edge_runs
//   corner lists  mesh_common.h's CSR whose lists ascend (mesh_corner_lists)
//   smoothing     one thread per vertex gathers through its corner list in ascending (f, j): a fixed order of fp64 basic operations,
//                 no float atomics -- the same bits from run to run and as the restatement                            k_mc_smooth
//   components    union-find over the runs (the larger root hooks under the smaller: a root is its component's lowest face), boxes by
//                 ordered-integer atomics behind a per-block reduction                                                k_mc_edge_runs, k_mc_labels, k_mc_comp_boxes
//                 (the box of all vertices: mesh_common.h's k_mesh_vertex_box)
//   rules 2-4     duplicates inside the run of a face's lowest edge, zero area at corner 0, incidences recounted over the survivors
//                                                                                                                     k_mc_duplicates, k_mc_classify, k_mc_nonmanifold
//   compaction    faces and the vertices they use, both renumbered in order (as the trim of k_poisson.hip)
// Built with -ffp-contract=off (csrc/Makefile): every fp64 expression below is evaluated as written.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"

#include <string.h>

#include <math.h>

#include <algorithm>
#include <vector>

namespace {

typedef unsigned long long u64;

enum { C_BAD_INDEX = 0, C_BAD_COORD, C_BORDER, C_COMPS, C_COMPS_DEAD, C_RM1, C_RM2, C_RM3, C_RM4, C_N };

// (the compiler turns a wave's adds of a constant into one add of its active-lane count)
__device__ __forceinline__ void count_if(bool flag, u64 *ctr) {
    if (flag) atomicAdd(ctr, (u64)1);
}

// ---- validation: every index in [0, nv), every coordinate finite --------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mc_validate(const float *__restrict__ v, size_t n_coords, const int32_t *__restrict__ f, size_t nv, size_t nf,
                                                     u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool bad_c = false, bad_i = false;
    if (i < n_coords) bad_c = !isfinite(v[i]);
    if (i < 3 * nf) bad_i = f[i] < 0 || (size_t)f[i] >= nv;
    count_if(bad_c, ctr + C_BAD_COORD);
    count_if(bad_i, ctr + C_BAD_INDEX);
}

// ---- the edge table (keys and union-find: mesh_common.h) -------------------------------------------------------------------------------
// one thread per sorted entry.  The first of a run counts the run (the edge's incidence), writes min(incidence, 3) to each of its
// entries' corners and marks both endpoints of an incidence-1 edge as border; every other entry unites its face with the one before.
__global__ __launch_bounds__(256) void k_mc_edge_runs(const u64 *__restrict__ key, const uint32_t *__restrict__ val, size_t n, u64 nv,
                                                      uint8_t *__restrict__ einc, uint8_t *__restrict__ vborder, int *__restrict__ parent) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    if ((k >> 32) == nv) return;
    if (i > 0 && key[i - 1] == k) {
        if (parent) uf_union(parent, (int)(val[i] / 3), (int)(val[i - 1] / 3));
        return;
    }
    if (!einc) return;
    size_t e = i + 1;
    while (e < n && key[e] == k) e++;
    const uint8_t inc = (uint8_t)(e - i > 3 ? 3 : e - i);
    for (size_t q = i; q < e; q++) einc[val[q]] = inc;
    if (inc == 1) vborder[k >> 32] = vborder[k & 0xffffffffu] = 1; // (every writer stores the same value)
}

// ---- smoothing ----------------------------------------------------------------------------------------------------------------------
// |(Pa - Pc) x (Pb - Pc)|^2 and (Pa - Pc) . (Pb - Pc), in the project's order (a0 b0 + a1 b1) + a2 b2
__device__ __forceinline__ double corner_n2(const D3 &pc, const D3 &pa, const D3 &pb, double *dot) {
    const double u0 = pa.x - pc.x, u1 = pa.y - pc.y, u2 = pa.z - pc.z;
    const double w0 = pb.x - pc.x, w1 = pb.y - pc.y, w2 = pb.z - pc.z;
    const double c0 = u1 * w2 - u2 * w1, c1 = u2 * w0 - u0 * w2, c2 = u0 * w1 - u1 * w0;
    *dot = (u0 * w0 + u1 * w1) + u2 * w2;
    return (c0 * c0 + c1 * c1) + c2 * c2;
}
// the cotangent at corner c of the triangle (c, a, b), clamped at 0; 0 for a corner without area
__device__ __forceinline__ double corner_weight(const D3 &pc, const D3 &pa, const D3 &pb) {
    double dot;
    const double n2 = corner_n2(pc, pa, pb, &dot);
    if (n2 == 0.0) return 0.0;
    const double c = dot / sqrt(n2);
    return c > 0.0 ? c : 0.0;
}

template <bool COT>
__global__ __launch_bounds__(256) void k_mc_smooth(const float *__restrict__ pin, float *__restrict__ pout, size_t nv, const int32_t *__restrict__ f,
                                                   const uint32_t *__restrict__ row, const uint32_t *__restrict__ corner, const uint8_t *__restrict__ einc,
                                                   const uint8_t *__restrict__ vborder, int boundary) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const D3 P = ld3(pin, (int)v);
    const bool border = vborder[v] != 0;
    if (border && !boundary) {
        for (int a = 0; a < 3; a++) pout[3 * v + a] = pin[3 * v + a];
        return;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0, W = 0.0;
    if (border) {
        sx = P.x;
        sy = P.y;
        sz = P.z;
        W = 1.0;
    }
    const uint32_t r0 = row[v], r1 = row[v + 1];
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t c = corner[r];
        const size_t fi = c / 3;
        const int j = (int)(c % 3);
        const int vi[3] = {f[3 * fi], f[3 * fi + 1], f[3 * fi + 2]};
        const int n1 = vi[(j + 1) % 3], n2 = vi[(j + 2) % 3];
        const D3 p1 = ld3(pin, n1), p2 = ld3(pin, n2);
        if (border) { // 1D: the other endpoint of every incidence-1 edge, weight 1
            if (einc[3 * fi + j] == 1) {
                sx += p1.x;
                sy += p1.y;
                sz += p1.z;
                W += 1.0;
            }
            if (einc[3 * fi + (j + 2) % 3] == 1) {
                sx += p2.x;
                sy += p2.y;
                sz += p2.z;
                W += 1.0;
            }
        } else { // neighbour v_j+1 with the weight of corner j+2, then v_j+2 with the weight of corner j+1
            const double w1 = COT ? corner_weight(p2, P, p1) : 1.0;
            sx += w1 * p1.x;
            sy += w1 * p1.y;
            sz += w1 * p1.z;
            W += w1;
            const double w2 = COT ? corner_weight(p1, p2, P) : 1.0;
            sx += w2 * p2.x;
            sy += w2 * p2.y;
            sz += w2 * p2.z;
            W += w2;
        }
    }
    const double d = 1.0 + W;
    pout[3 * v] = (float)((P.x + sx) / d);
    pout[3 * v + 1] = (float)((P.y + sy) / d);
    pout[3 * v + 2] = (float)((P.z + sz) / d);
}

__global__ __launch_bounds__(256) void k_mc_count_u8(const uint8_t *__restrict__ a, size_t n, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    count_if(i < n && a[i] != 0, ctr);
}

// ---- components ---------------------------------------------------------------------------------------------------------------------
// label = the root (the lowest face of the component); -1 for a face with a repeated index.  (Runs after every union, in a launch of its own.)
__global__ __launch_bounds__(256) void k_mc_labels(const int32_t *__restrict__ f, size_t nf, int *__restrict__ parent, int32_t *__restrict__ label, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool root = false;
    if (i < nf) {
        const bool ok = face_distinct(f[3 * i], f[3 * i + 1], f[3 * i + 2]);
        const int r = ok ? uf_find(parent, (int)i) : -1;
        label[i] = r;
        root = r == (int)i;
    }
    count_if(root, ctr + C_COMPS);
}

// box[6 c .. 6 c + 5] = min x, y, z, max x, y, z (ordered uints) of component c's faces, box[6 nf ..] that of all vertices.  One giant
// component is the contention case: the threads of a block that share thread 0's label reduce in LDS first, one atomic per block and bound.
__global__ __launch_bounds__(256) void k_mc_comp_boxes(const float *__restrict__ p, const int32_t *__restrict__ f, size_t nf, const int32_t *__restrict__ label,
                                                       unsigned int *__restrict__ box) {
    __shared__ unsigned int s_mm[6];
    __shared__ int s_lab;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lab = i < nf ? label[i] : -1;
    if (threadIdx.x == 0) s_lab = lab;
    if (threadIdx.x < 6) s_mm[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    if (lab >= 0) {
        unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
        for (int c = 0; c < 3; c++) {
            const size_t v = (size_t)f[3 * i + c];
            for (int a = 0; a < 3; a++) {
                const unsigned int o = f2ord(p[3 * v + a]);
                lo[a] = o < lo[a] ? o : lo[a];
                hi[a] = o > hi[a] ? o : hi[a];
            }
        }
        unsigned int *dst = lab == s_lab ? s_mm : box + 6 * (size_t)lab;
        for (int a = 0; a < 3; a++) {
            atomicMin(dst + a, lo[a]);
            atomicMax(dst + 3 + a, hi[a]);
        }
    }
    __syncthreads();
    if (s_lab >= 0 && threadIdx.x < 6) {
        unsigned int *dst = box + 6 * (size_t)s_lab + threadIdx.x;
        if (threadIdx.x < 3) atomicMin(dst, s_mm[threadIdx.x]);
        else atomicMax(dst, s_mm[threadIdx.x]);
    }
}
__global__ __launch_bounds__(256) void k_mc_box_init(unsigned int *__restrict__ box, size_t n6) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n6) box[i] = (i % 6) < 3 ? 0xffffffffu : 0u;
}
// a component goes when the fp64 diameter of its float32 box is below the threshold (strictly)
__global__ __launch_bounds__(256) void k_mc_comp_dead(const int32_t *__restrict__ label, size_t nf, const unsigned int *__restrict__ box, double threshold,
                                                      uint8_t *__restrict__ dead, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool d = false;
    if (i < nf) {
        if (label[i] == (int)i) {
            d = sqrt(box_diagonal2(box + 6 * i)) < threshold;
        }
        dead[i] = d ? 1 : 0;
    }
    count_if(d, ctr + C_COMPS_DEAD);
}

// ---- rules 2 - 4 --------------------------------------------------------------------------------------------------------------------
// Faces with the same three vertices share every edge, so they meet in the run of their lowest edge (the two smaller vertices), where the
// stable sort left them in ascending face order: a face is a duplicate when an earlier entry of that run has its third vertex.
__global__ __launch_bounds__(256) void k_mc_duplicates(const u64 *__restrict__ key, const uint32_t *__restrict__ val, size_t n, u64 nv, const int32_t *__restrict__ f,
                                                       uint8_t *__restrict__ dup) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    if ((k >> 32) == nv) return;
    const uint32_t c = val[i];
    const int32_t t = f[3 * (size_t)(c / 3) + (c % 3 + 2) % 3];
    if ((u64)t < (k & 0xffffffffu)) return; // (not this face's lowest edge)
    for (size_t q = i; q > 0 && key[q - 1] == k; q--) {
        const uint32_t g = val[q - 1];
        if (f[3 * (size_t)(g / 3) + (g % 3 + 2) % 3] == t) {
            dup[c / 3] = 1;
            return;
        }
    }
}

// rules 1 - 3 in script2's order: each rule sees the faces the rules before it left
__global__ __launch_bounds__(256) void k_mc_classify(const float *__restrict__ p, const int32_t *__restrict__ f, size_t nf, const int32_t *__restrict__ label,
                                                     const uint8_t *__restrict__ dead, const uint8_t *__restrict__ dup, unsigned flags, uint8_t *__restrict__ alive,
                                                     u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool r1 = false, r2 = false, r3 = false;
    if (i < nf) {
        const int lab = label[i];
        r1 = lab >= 0 && dead[lab];
        bool live = !r1;
        r2 = live && (flags & RSM_MESH_CLEAN_DUPLICATES) && dup[i];
        live = live && !r2;
        if (live && (flags & RSM_MESH_CLEAN_ZERO_AREA)) {
            const int a = f[3 * i], b = f[3 * i + 1], c = f[3 * i + 2];
            if (!face_distinct(a, b, c)) r3 = true;
            else {
                double dot;
                r3 = corner_n2(ld3(p, a), ld3(p, b), ld3(p, c), &dot) == 0.0;
            }
        }
        alive[i] = live && !r3;
    }
    count_if(r1, ctr + C_RM1);
    count_if(r2, ctr + C_RM2);
    count_if(r3, ctr + C_RM3);
}

// rule 4: the first entry of a run counts the run's faces that are still alive; more than two: all of them go
__global__ __launch_bounds__(256) void k_mc_nonmanifold(const u64 *__restrict__ key, const uint32_t *__restrict__ val, size_t n, u64 nv, const uint8_t *__restrict__ alive,
                                                        uint8_t *__restrict__ nm) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    if ((k >> 32) == nv || (i > 0 && key[i - 1] == k)) return;
    size_t e = i, cnt = 0;
    for (; e < n && key[e] == k; e++) cnt += alive[val[e] / 3];
    if (cnt <= 2) return;
    for (size_t q = i; q < e; q++)
        if (alive[val[q] / 3]) nm[val[q] / 3] = 1; // (every writer stores the same value)
}

__global__ __launch_bounds__(256) void k_mc_keep(const int32_t *__restrict__ f, size_t nf, const uint8_t *__restrict__ alive, const uint8_t *__restrict__ nm, unsigned flags,
                                                 unsigned int *__restrict__ fkeep, unsigned int *__restrict__ vused, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool r4 = false;
    if (i < nf) {
        r4 = alive[i] && (flags & RSM_MESH_CLEAN_NONMANIFOLD) && nm[i];
        const unsigned int keep = alive[i] && !r4 ? 1u : 0u;
        fkeep[i] = keep;
        if (keep) vused[f[3 * i]] = vused[f[3 * i + 1]] = vused[f[3 * i + 2]] = 1u; // (every writer stores the same value)
    }
    count_if(r4, ctr + C_RM4);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// what the stages share: counters, the sorted edge table, and (on request) incidences, border flags, the union-find forest
struct Tables {
    u64 *ctr = nullptr;     // C_N counters
    u64 *ekey = nullptr;    // 3 nf sorted keys
    uint32_t *eval = nullptr;
    uint8_t *einc = nullptr, *vborder = nullptr;
    int *parent = nullptr;
};

// RSM_OK, or RSM_E_INVALID with *what = 1 (an index out of range) / 2 (a coordinate not finite)
static int validate(DevMem &M, Tables &T, const float *d_v, size_t nv, const int32_t *d_f, size_t nf, int *what, hipStream_t st) {
    T.ctr = M.get<u64>(C_N);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(T.ctr, 0, C_N * sizeof(u64), st));
    const size_t n_coords = d_v ? 3 * nv : 0, n = std::max(n_coords, 3 * nf);
    if (n > 0) hipLaunchKernelGGL(k_mc_validate, blocks_for(n), dim3(256), 0, st, d_v, n_coords, d_f, nv, nf, T.ctr);
    u64 h[2] = {0, 0};
    DEVCHK(hipMemcpyAsync(h, T.ctr, sizeof h, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    *what = h[C_BAD_INDEX] ? 1 : h[C_BAD_COORD] ? 2 : 0;
    return *what ? RSM_E_INVALID : RSM_OK;
}

// the sorted edge table of nf > 0 faces; want_inc: einc and vborder, want_uf: the forest after every union
static int edge_table(DevMem &M, Tables &T, const int32_t *d_f, size_t nv, size_t nf, bool want_inc, bool want_uf, hipStream_t st) {
    const size_t n = 3 * nf;
    u64 *k0 = M.get<u64>(n);
    uint32_t *v0 = M.get<uint32_t>(n);
    T.ekey = M.get<u64>(n);
    T.eval = M.get<uint32_t>(n);
    if (want_inc) {
        T.einc = M.get<uint8_t>(n);
        T.vborder = M.get<uint8_t>(nv);
    }
    if (want_uf) T.parent = M.get<int>(nf);
    if (!M.ok) return RSM_E_NOMEM;
    const int s = mesh_edge_table(M, d_f, nv, nf, k0, v0, T.ekey, T.eval, st);
    if (s != RSM_OK) return s;
    if (want_inc) {
        DEVCHK(hipMemsetAsync(T.einc, 0, n, st));
        DEVCHK(hipMemsetAsync(T.vborder, 0, nv ? nv : 1, st));
    }
    if (want_uf) hipLaunchKernelGGL(k_mesh_iota<>, blocks_for(nf), dim3(256), 0, st, T.parent, nf);
    hipLaunchKernelGGL(k_mc_edge_runs, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, (const uint32_t *)T.eval, n, (u64)nv, T.einc, T.vborder, T.parent);
    return RSM_OK;
}

// `steps` simultaneous steps from d_in; the result is in *d_res (d_in itself with steps = 0, else one of the two scratch buffers)
static int smooth(DevMem &M, const Tables &T, const float *d_in, size_t nv, const int32_t *d_f, size_t nf, int steps, int cotangent, int boundary,
                  const float **d_res, hipStream_t st) {
    *d_res = d_in;
    if (steps <= 0 || nv == 0 || nf == 0) return RSM_OK;
    uint32_t *corner = nullptr, *row = nullptr;
    const int s = mesh_corner_lists(M, d_f, nv, nf, &row, &corner, st);
    if (s != RSM_OK) return s;
    float *buf[2] = {M.get<float>(3 * nv), M.get<float>(3 * nv)};
    if (!M.ok) return RSM_E_NOMEM;
    const float *src = d_in;
    for (int it = 0; it < steps; it++) {
        float *dst = buf[it & 1];
        if (cotangent)
            hipLaunchKernelGGL(k_mc_smooth<true>, blocks_for(nv), dim3(256), 0, st, src, dst, nv, d_f, (const uint32_t *)row, (const uint32_t *)corner,
                               (const uint8_t *)T.einc, (const uint8_t *)T.vborder, boundary);
        else
            hipLaunchKernelGGL(k_mc_smooth<false>, blocks_for(nv), dim3(256), 0, st, src, dst, nv, d_f, (const uint32_t *)row, (const uint32_t *)corner,
                               (const uint8_t *)T.einc, (const uint8_t *)T.vborder, boundary);
        src = dst;
    }
    *d_res = src;
    return RSM_OK;
}

} // namespace

int mesh_validate_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, int *invalid, hipStream_t st) {
    DevMem M;
    Tables T;
    return validate(M, T, d_v, (size_t)nv, d_f, (size_t)nf, invalid, st);
}

int mesh_smooth_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, int steps, int cotangent, int boundary, float *d_out, int64_t *n_border,
                       int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    *n_border = 0;
    DevMem M;
    Tables T;
    int s = validate(M, T, d_v, nv, d_f, nf, invalid, st);
    if (s != RSM_OK) return s;
    const float *res = d_v;
    if (nf > 0 && nv > 0) {
        if ((s = edge_table(M, T, d_f, nv, nf, true, false, st)) != RSM_OK) return s;
        hipLaunchKernelGGL(k_mc_count_u8, blocks_for(nv), dim3(256), 0, st, (const uint8_t *)T.vborder, nv, T.ctr + C_BORDER);
        if ((s = smooth(M, T, d_v, nv, d_f, nf, steps, cotangent, boundary, &res, st)) != RSM_OK) return s;
    }
    if (nv > 0) DEVCHK(hipMemcpyAsync(d_out, res, 3 * nv * sizeof(float), hipMemcpyDeviceToDevice, st));
    u64 h[C_N];
    DEVCHK(hipMemcpyAsync(h, T.ctr, sizeof h, hipMemcpyDeviceToHost, st));
    if ((s = mesh_finish(st)) != RSM_OK) return s;
    *n_border = (int64_t)h[C_BORDER];
    return RSM_OK;
}

int mesh_components_device(const int32_t *d_f, int64_t nv_, int64_t nf_, int32_t *d_label, int64_t *n_components, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    *n_components = 0;
    DevMem M;
    Tables T;
    int s = validate(M, T, nullptr, nv, d_f, nf, invalid, st);
    if (s != RSM_OK || nf == 0) return s;
    if ((s = edge_table(M, T, d_f, nv, nf, false, true, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_mc_labels, blocks_for(nf), dim3(256), 0, st, d_f, nf, T.parent, d_label, T.ctr);
    u64 h[C_N];
    DEVCHK(hipMemcpyAsync(h, T.ctr, sizeof h, hipMemcpyDeviceToHost, st));
    if ((s = mesh_finish(st)) != RSM_OK) return s;
    *n_components = (int64_t)h[C_COMPS];
    return RSM_OK;
}

int mesh_clean_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const rsm_mesh_clean_params *p, PoissonMesh *out, double *stats, int *invalid,
                      hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    double S[RSM_MESH_CLEAN_STATS] = {0};
    S[0] = (double)nv;
    S[1] = (double)nf;
    DevMem M;
    Tables T;
    PoissonMesh res;
    int s = validate(M, T, d_v, nv, d_f, nf, invalid, st);
    if (s != RSM_OK) return s;
    const float *pos = d_v;
    const bool work = nv > 0 && nf > 0;
    if (work) {
        if ((s = edge_table(M, T, d_f, nv, nf, true, true, st)) != RSM_OK) return s;
        hipLaunchKernelGGL(k_mc_count_u8, blocks_for(nv), dim3(256), 0, st, (const uint8_t *)T.vborder, nv, T.ctr + C_BORDER);
        if ((s = smooth(M, T, d_v, nv, d_f, nf, p->smooth_steps, p->cotangent, p->boundary, &pos, st)) != RSM_OK) return s;
    }
    // D: the diameter of the box of all nv (smoothed) vertices
    unsigned int *box = M.get<unsigned int>(6 * (nf + 1));
    if (!M.ok) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_mc_box_init, blocks_for(6 * (nf + 1)), dim3(256), 0, st, box, 6 * (nf + 1));
    double D = 0.0;
    if (nv > 0) {
        unsigned int h[6];
        hipLaunchKernelGGL(k_mesh_vertex_box<>, dim3((unsigned)std::min<size_t>(1024, (nv + 255) / 256)), dim3(256), 0, st, pos, nv, box + 6 * nf);
        DEVCHK(hipMemcpyAsync(h, box + 6 * nf, sizeof h, hipMemcpyDeviceToHost, st));
        if ((s = mesh_finish(st)) != RSM_OK) return s;
        D = sqrt(box_diagonal2(h));
    }
    const double threshold = p->min_piece_relative ? p->min_piece * D : p->min_piece;
    S[12] = D;
    S[13] = threshold;
    if (work) {
        const size_t n = 3 * nf;
        int32_t *label = M.get<int32_t>(nf);
        uint8_t *dead = M.get<uint8_t>(nf), *dup = M.get<uint8_t>(nf), *alive = M.get<uint8_t>(nf), *nm = M.get<uint8_t>(nf);
        unsigned int *fkeep = M.get<unsigned int>(nf), *fpos = M.get<unsigned int>(nf), *vused = M.get<unsigned int>(nv), *vpos = M.get<unsigned int>(nv);
        if (!M.ok) return RSM_E_NOMEM;
        DEVCHK(hipMemsetAsync(dup, 0, nf, st));
        DEVCHK(hipMemsetAsync(nm, 0, nf, st));
        DEVCHK(hipMemsetAsync(vused, 0, nv * sizeof(unsigned int), st));
        hipLaunchKernelGGL(k_mc_labels, blocks_for(nf), dim3(256), 0, st, d_f, nf, T.parent, label, T.ctr);
        hipLaunchKernelGGL(k_mc_comp_boxes, blocks_for(nf), dim3(256), 0, st, pos, d_f, nf, (const int32_t *)label, box);
        hipLaunchKernelGGL(k_mc_comp_dead, blocks_for(nf), dim3(256), 0, st, (const int32_t *)label, nf, (const unsigned int *)box, threshold, dead, T.ctr);
        if (p->flags & RSM_MESH_CLEAN_DUPLICATES)
            hipLaunchKernelGGL(k_mc_duplicates, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, (const uint32_t *)T.eval, n, (u64)nv, d_f, dup);
        hipLaunchKernelGGL(k_mc_classify, blocks_for(nf), dim3(256), 0, st, pos, d_f, nf, (const int32_t *)label, (const uint8_t *)dead, (const uint8_t *)dup, p->flags,
                           alive, T.ctr);
        if (p->flags & RSM_MESH_CLEAN_NONMANIFOLD)
            hipLaunchKernelGGL(k_mc_nonmanifold, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, (const uint32_t *)T.eval, n, (u64)nv, (const uint8_t *)alive, nm);
        hipLaunchKernelGGL(k_mc_keep, blocks_for(nf), dim3(256), 0, st, d_f, nf, (const uint8_t *)alive, (const uint8_t *)nm, p->flags, fkeep, vused, T.ctr);
        if ((s = scan_u32(M, (const unsigned int *)fkeep, fpos, nf, st)) != RSM_OK || (s = scan_u32(M, (const unsigned int *)vused, vpos, nv, st)) != RSM_OK) return s;
        uint64_t kf = 0, kv = 0;
        if ((s = scan_totals(fkeep, fpos, nf, vused, vpos, nv, st, &kf, &kv)) != RSM_OK) return s;
        if (kf > 0) {
            if ((s = mesh_result_alloc(res, kv, kf)) != RSM_OK) return s;
            hipLaunchKernelGGL(k_mesh_compact_faces<>, blocks_for(nf), dim3(256), 0, st, d_f, nf, (const unsigned int *)fkeep, (const unsigned int *)fpos,
                               (const unsigned int *)vpos, res.d_f);
            hipLaunchKernelGGL(k_mesh_compact_verts<>, blocks_for(nv), dim3(256), 0, st, pos, nv, (const unsigned int *)vused, (const unsigned int *)vpos, res.d_v);
        }
    }
    u64 h[C_N];
    if (hipMemcpyAsync(h, T.ctr, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess || mesh_finish(st) != RSM_OK) {
        poisson_mesh_free(&res);
        return RSM_E_HIP;
    }
    S[2] = (double)res.nv;
    S[3] = (double)res.nf;
    S[4] = (double)h[C_BORDER];
    S[5] = (double)h[C_COMPS];
    S[6] = (double)h[C_COMPS_DEAD];
    S[7] = (double)h[C_RM1];
    S[8] = (double)h[C_RM2];
    S[9] = (double)h[C_RM3];
    S[10] = (double)h[C_RM4];
    S[11] = (double)(nv - (size_t)res.nv);
    if (stats) memcpy(stats, S, sizeof S);
    mesh_result_commit(out, res);
    return RSM_OK;
}
