// k_meshclose.hip -- script2.mlx's last filter, "Close Holes" (MaxHoleSize 30), on the cleaned surface.  Not a bit-parity
// port of MeshLab / VCG (no source in the reference tree): every rule is defined in DESIGN.md 9 (f12) and restated in numpy in
// tests/meshclose_restatement.py, and the kernels are held to that restatement exactly -- the same faces in the same order.
//   border        the sorted edge table of mesh_common.h; an entry whose run has length 1 is a border entry, directed as its face
//                 (tail v_j, head v_j+1); per vertex the border entries that leave / reach it are counted by integer atomics, and the one
//                 entry of a simple vertex (one in, one out) is recorded by a plain store                          k_ch_border
//   components    union-find over the entries (mesh_common.h): e joins the entry that leaves its head when the head is simple; size and
//                 the "open" mark (a head that is not simple) go to the root, the lowest entry                     k_ch_link, k_ch_roots
//   eligible      loops of at most max_hole_size entries that are not a lone triangle, compacted in ascending label k_ch_classify, k_ch_list
//   fill          one wave per hole: the ring and its fp64 positions, the forbidden diagonals (binary searches in the sorted keys), the
//                 least-area table W / K span by span in LDS, the triangles in the pre-order of the recursion       k_ch_fill
//   output        vertices and faces copied, the new faces appended at the scanned offsets                          k_ch_gather
// fp64 + - * / sqrt only, no float atomics; built with -ffp-contract=off (csrc/Makefile): every expression is evaluated as written.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"

#include <string.h>

#include <math.h>

#include <algorithm>

namespace {

typedef unsigned long long u64;

enum { H_BORDER = 0, H_COMPS, H_LOOPS, H_OPEN, H_CLOSED, H_LONG, H_LONE, H_NOTRI, H_LMAX_CLOSED, H_LMAX_SEEN, H_LMAX_ELIGIBLE, H_N };

// ---- border entries -------------------------------------------------------------------------------------------------------------------------
// one thread per sorted position: a run of length 1 is a border entry
__global__ __launch_bounds__(256) void k_ch_border(const u64 *__restrict__ key, const uint32_t *__restrict__ val, size_t n, u64 nv, const int32_t *__restrict__ f,
                                                   uint8_t *__restrict__ isb, int *__restrict__ n_in, int *__restrict__ n_out, int *__restrict__ in_entry,
                                                   int *__restrict__ out_entry, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    if ((k >> 32) == nv) return;
    if ((i > 0 && key[i - 1] == k) || (i + 1 < n && key[i + 1] == k)) return;
    const uint32_t e = val[i];
    const size_t fi = e / 3;
    const int j = (int)(e % 3);
    const int t = f[3 * fi + j], h = f[3 * fi + (j + 1) % 3];
    isb[e] = 1;
    atomicAdd(n_out + t, 1);
    atomicAdd(n_in + h, 1);
    out_entry[t] = (int)e; // (read only where the vertex is simple: then this is the one writer)
    in_entry[h] = (int)e;
    atomicAdd(ctr + H_BORDER, (u64)1);
}

__device__ __forceinline__ int entry_head(const int32_t *__restrict__ f, size_t e) { return f[3 * (e / 3) + (e % 3 + 1) % 3]; }
__device__ __forceinline__ int entry_tail(const int32_t *__restrict__ f, size_t e) { return f[e]; }

__global__ __launch_bounds__(256) void k_ch_link(const int32_t *__restrict__ f, size_t n, const uint8_t *__restrict__ isb, const int *__restrict__ n_in,
                                                 const int *__restrict__ n_out, const int *__restrict__ out_entry, int *__restrict__ parent) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n || !isb[e]) return;
    const int h = entry_head(f, e);
    if (n_in[h] == 1 && n_out[h] == 1) uf_union(parent, (int)e, out_entry[h]);
}

// label = the root (the lowest entry of the component), -1 for an entry that is no border entry; size and the open mark on the root.
// (Runs after every union, in a launch of its own.)
__global__ __launch_bounds__(256) void k_ch_roots(const int32_t *__restrict__ f, size_t n, const uint8_t *__restrict__ isb, const int *__restrict__ n_in,
                                                  const int *__restrict__ n_out, int *__restrict__ parent, int32_t *__restrict__ label, int *__restrict__ csize,
                                                  int *__restrict__ copen) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    if (!isb[e]) {
        label[e] = -1;
        return;
    }
    const int r = uf_find(parent, (int)e);
    label[e] = r;
    atomicAdd(csize + r, 1);
    const int h = entry_head(f, e);
    if (!(n_in[h] == 1 && n_out[h] == 1)) atomicOr(copen + r, 1);
}

// one thread per entry; a root classifies its component
__global__ __launch_bounds__(256) void k_ch_classify(size_t n, const int32_t *__restrict__ label, const int *__restrict__ csize, const int *__restrict__ copen,
                                                     int max_hole, unsigned int *__restrict__ elig, u64 *__restrict__ ctr) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    unsigned int el = 0u;
    if (label[e] == (int)e) {
        atomicAdd(ctr + H_COMPS, (u64)1);
        if (copen[e]) {
            atomicAdd(ctr + H_OPEN, (u64)1);
        } else {
            const int L = csize[e];
            atomicAdd(ctr + H_LOOPS, (u64)1);
            atomicMax(ctr + H_LMAX_SEEN, (u64)L);
            // a lone triangle: the three entries of one face (the root is then its corner 0)
            const bool lone = L == 3 && e % 3 == 0 && label[e + 1] == (int)e && label[e + 2] == (int)e;
            if (L > max_hole) atomicAdd(ctr + H_LONG, (u64)1);
            else if (lone) atomicAdd(ctr + H_LONE, (u64)1);
            else {
                el = 1u;
                atomicMax(ctr + H_LMAX_ELIGIBLE, (u64)L);
            }
        }
    }
    elig[e] = el;
}

// the stage's view: per entry L for a loop's, 0 for an open component's, -1 otherwise
__global__ __launch_bounds__(256) void k_ch_sizes(size_t n, const int32_t *__restrict__ label, const int *__restrict__ csize, const int *__restrict__ copen,
                                                  int32_t *__restrict__ size) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int r = label[e];
    size[e] = r < 0 ? -1 : copen[r] ? 0 : csize[r];
}

__global__ __launch_bounds__(256) void k_ch_list(size_t n, const unsigned int *__restrict__ elig, const unsigned int *__restrict__ epos, int *__restrict__ hole) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n && elig[e]) hole[epos[e]] = (int)e;
}

// ---- the fill: one wave per hole ------------------------------------------------------------------------------------------------------------
// LM = the longest ring this instance holds (the table is LM x LM).  Mesh mode (ring_xyz == NULL): hole h is the loop rooted at hole[h], its
// ring walked through in_entry, its forbidden diagonals looked up in the sorted keys, its triangles written as vertex indices.  Stage mode:
// one ring of stage_L points at ring_xyz, forbidden pairs from mask (stage_L x stage_L bytes, may be NULL), triangles as ring positions.
// tri: stride triangles per hole; nadd[h] = the triangles written (L - 2, or 0 when W(0, L-1) = +inf), wout (may be NULL) = W(0, L-1).
template <int LM>
__global__ __launch_bounds__(64) void k_ch_fill(const float *__restrict__ v, const int32_t *__restrict__ f, const u64 *__restrict__ ekey, size_t n,
                                                const int *__restrict__ in_entry, const int *__restrict__ hole, const int *__restrict__ csize,
                                                const float *__restrict__ ring_xyz, const uint8_t *__restrict__ mask, int stage_L, int stride,
                                                int32_t *__restrict__ tri, unsigned int *__restrict__ nadd, double *__restrict__ wout, u64 *__restrict__ ctr) {
    constexpr int LS = LM + 1; // (a row's stride: lanes over i read W[i][k] at the same k without sharing a bank)
    __shared__ double W[LM * LS];
    __shared__ double P[LM * 3];
    __shared__ int R[LM];
    __shared__ signed char K[LM * LM]; // -2 before the table: a forbidden diagonal
    __shared__ unsigned char stk[2 * LM];
    const size_t h = blockIdx.x;
    const int lane = (int)threadIdx.x;
    const bool stage = ring_xyz != nullptr;
    const int e0 = stage ? 0 : hole[h];
    const int L = stage ? stage_L : csize[e0];
    if (L < 3 || L > LM || L - 2 > stride) { // (the host sizes LM and stride by the longest eligible loop)
        if (lane == 0) nadd[h] = 0u;
        return;
    }
    if (!stage && lane == 0) { // the border against the faces' direction
        int r = entry_tail(f, (size_t)e0);
        R[0] = entry_head(f, (size_t)e0);
        R[1] = r;
        for (int t = 2; t < L; t++) {
            r = entry_tail(f, (size_t)in_entry[r]);
            R[t] = r;
        }
    }
    if (stage && lane < L) R[lane] = lane;
    __syncthreads();
    if (lane < L) {
        const float *src = stage ? ring_xyz : v;
        const size_t q = (size_t)R[lane];
        for (int a = 0; a < 3; a++) P[3 * lane + a] = (double)src[3 * q + a];
    }
    for (int p = lane; p < L * L; p += 64) {
        const int i = p / L, j = p % L;
        signed char kk = -1;
        if (j >= i + 2 && !(i == 0 && j == L - 1)) {
            bool forb;
            if (stage) {
                forb = mask != nullptr && mask[p] != 0;
            } else {
                const u64 a = (u64)R[i], b = (u64)R[j];
                const u64 want = (a < b ? a : b) << 32 | (a < b ? b : a);
                size_t lo = 0, hi = n;
                while (lo < hi) {
                    const size_t mid = (lo + hi) / 2;
                    if (ekey[mid] < want) lo = mid + 1;
                    else hi = mid;
                }
                forb = lo < n && ekey[lo] == want;
            }
            if (forb) kk = -2;
        }
        K[i * LM + j] = kk;
        if (j == i + 1) W[i * LS + j] = 0.0;
    }
    __syncthreads();
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int s = 2; s < L; s++) {
        const int i = lane, j = lane + s;
        if (j < L) {
            double best = inf;
            int bk = -1;
            if (K[i * LM + j] != -2) {
                const double pi0 = P[3 * i], pi1 = P[3 * i + 1], pi2 = P[3 * i + 2];
                const double w0 = P[3 * j] - pi0, w1 = P[3 * j + 1] - pi1, w2 = P[3 * j + 2] - pi2;
                for (int k = i + 1; k < j; k++) {
                    const double u0 = P[3 * k] - pi0, u1 = P[3 * k + 1] - pi1, u2 = P[3 * k + 2] - pi2;
                    const double c0 = u1 * w2 - u2 * w1, c1 = u2 * w0 - u0 * w2, c2 = u0 * w1 - u1 * w0;
                    const double n2 = (c0 * c0 + c1 * c1) + c2 * c2;
                    const double A = n2 == 0.0 ? inf : 0.5 * sqrt(n2);
                    const double c = (W[i * LS + k] + W[k * LS + j]) + A;
                    if (c < best) {
                        best = c;
                        bk = k;
                    }
                }
            }
            W[i * LS + j] = best;
            K[i * LM + j] = (signed char)bk;
        }
        __syncthreads();
    }
    if (lane != 0) return;
    const double w = W[L - 1];
    if (wout) wout[h] = w;
    // emit(0, L - 1) in pre-order; the stack holds spans of at least 2 only, each of which still owes a triangle: never more than L - 2
    int t = 0;
    if (w < inf) {
        int32_t *out = tri + 3 * (size_t)stride * h;
        int sp = 1;
        stk[0] = 0;
        stk[1] = (unsigned char)(L - 1);
        while (sp > 0 && t < L - 2) {
            sp--;
            const int i = stk[2 * sp], j = stk[2 * sp + 1];
            const int k = K[i * LM + j];
            if (k <= i || k >= j) { // (cannot be: a finite W(i, j) has its k, and so have both parts; the hole would stay whole)
                t = 0;
                break;
            }
            out[3 * t] = R[i];
            out[3 * t + 1] = R[k];
            out[3 * t + 2] = R[j];
            t++;
            if (j - k >= 2) {
                stk[2 * sp] = (unsigned char)k;
                stk[2 * sp + 1] = (unsigned char)j;
                sp++;
            }
            if (k - i >= 2) {
                stk[2 * sp] = (unsigned char)i;
                stk[2 * sp + 1] = (unsigned char)k;
                sp++;
            }
        }
    }
    const bool ok = t == L - 2; // what was written is what the gather copies
    nadd[h] = ok ? (unsigned int)t : 0u;
    if (ctr) {
        if (ok) {
            atomicAdd(ctr + H_CLOSED, (u64)1);
            atomicMax(ctr + H_LMAX_CLOSED, (u64)L);
        } else {
            atomicAdd(ctr + H_NOTRI, (u64)1);
        }
    }
}

// the new faces behind the input's: hole h's nadd[h] triangles at off[h]
__global__ __launch_bounds__(256) void k_ch_gather(size_t total, int stride, const unsigned int *__restrict__ nadd, const unsigned int *__restrict__ off,
                                                   const int32_t *__restrict__ tri, int32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t h = i / (size_t)stride;
    const unsigned int t = (unsigned int)(i % (size_t)stride);
    if (t >= nadd[h]) return;
    const size_t o = (size_t)off[h] + t;
    for (int c = 0; c < 3; c++) out[3 * o + c] = tri[3 * i + c];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
struct Loops {
    u64 *ctr = nullptr, *ekey = nullptr;
    uint32_t *eval = nullptr;
    uint8_t *isb = nullptr;
    int *n_in = nullptr, *n_out = nullptr, *in_entry = nullptr, *out_entry = nullptr, *parent = nullptr, *csize = nullptr, *copen = nullptr;
    int32_t *label = nullptr;
};

// rules 2-3 on a validated mesh with nv > 0 and nf > 0: the sorted table, the border entries, the components with size and open mark
static int border_loops(DevMem &M, Loops &T, const int32_t *d_f, size_t nv, size_t nf, hipStream_t st) {
    const size_t n = 3 * nf;
    u64 *k0 = M.get<u64>(n);
    uint32_t *v0 = M.get<uint32_t>(n);
    T.ctr = M.get<u64>(H_N);
    T.ekey = M.get<u64>(n);
    T.eval = M.get<uint32_t>(n);
    T.isb = M.get<uint8_t>(n);
    T.n_in = M.get<int>(nv);
    T.n_out = M.get<int>(nv);
    T.in_entry = M.get<int>(nv);
    T.out_entry = M.get<int>(nv);
    T.parent = M.get<int>(n);
    T.csize = M.get<int>(n);
    T.copen = M.get<int>(n);
    T.label = M.get<int32_t>(n);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(T.ctr, 0, H_N * sizeof(u64), st));
    DEVCHK(hipMemsetAsync(T.isb, 0, n, st));
    DEVCHK(hipMemsetAsync(T.n_in, 0, nv * sizeof(int), st));
    DEVCHK(hipMemsetAsync(T.n_out, 0, nv * sizeof(int), st));
    DEVCHK(hipMemsetAsync(T.in_entry, 0, nv * sizeof(int), st));
    DEVCHK(hipMemsetAsync(T.out_entry, 0, nv * sizeof(int), st));
    DEVCHK(hipMemsetAsync(T.csize, 0, n * sizeof(int), st));
    DEVCHK(hipMemsetAsync(T.copen, 0, n * sizeof(int), st));
    const int s = mesh_edge_table(M, d_f, nv, nf, k0, v0, T.ekey, T.eval, st);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL(k_ch_border, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, (const uint32_t *)T.eval, n, (u64)nv, d_f, T.isb, T.n_in, T.n_out, T.in_entry,
                       T.out_entry, T.ctr);
    hipLaunchKernelGGL(k_mesh_iota<>, blocks_for(n), dim3(256), 0, st, T.parent, n);
    hipLaunchKernelGGL(k_ch_link, blocks_for(n), dim3(256), 0, st, d_f, n, (const uint8_t *)T.isb, (const int *)T.n_in, (const int *)T.n_out, (const int *)T.out_entry,
                       T.parent);
    hipLaunchKernelGGL(k_ch_roots, blocks_for(n), dim3(256), 0, st, d_f, n, (const uint8_t *)T.isb, (const int *)T.n_in, (const int *)T.n_out, T.parent, T.label, T.csize,
                       T.copen);
    return RSM_OK;
}

// the instance whose table holds rings of up to lmax points (3 .. RSM_MESH_CLOSE_MAX_HOLE): 16, 32 or 64 -- the same result from each
static void launch_fill(int lmax, size_t holes, const float *d_v, const int32_t *d_f, const Loops &T, size_t n, const int *hole, const float *d_ring,
                        const uint8_t *d_mask, int stage_L, int stride, int32_t *tri, unsigned int *nadd, double *wout, u64 *ctr, hipStream_t st) {
    const dim3 grid((unsigned)holes), block(64);
    if (lmax <= 16)
        hipLaunchKernelGGL(k_ch_fill<16>, grid, block, 0, st, d_v, d_f, (const u64 *)T.ekey, n, (const int *)T.in_entry, hole, (const int *)T.csize, d_ring, d_mask, stage_L,
                           stride, tri, nadd, wout, ctr);
    else if (lmax <= 32)
        hipLaunchKernelGGL(k_ch_fill<32>, grid, block, 0, st, d_v, d_f, (const u64 *)T.ekey, n, (const int *)T.in_entry, hole, (const int *)T.csize, d_ring, d_mask, stage_L,
                           stride, tri, nadd, wout, ctr);
    else
        hipLaunchKernelGGL(k_ch_fill<64>, grid, block, 0, st, d_v, d_f, (const u64 *)T.ekey, n, (const int *)T.in_entry, hole, (const int *)T.csize, d_ring, d_mask, stage_L,
                           stride, tri, nadd, wout, ctr);
}

} // namespace

int mesh_border_loops_device(const int32_t *d_f, int64_t nv_, int64_t nf_, int32_t *d_label, int32_t *d_size, int64_t *n_components, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_, n = 3 * nf;
    *n_components = 0;
    int s = mesh_validate_device(nullptr, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK || nf == 0) return s;
    DevMem M;
    Loops T;
    if ((s = border_loops(M, T, d_f, nv, nf, st)) != RSM_OK) return s;
    unsigned int *elig = M.get<unsigned int>(n);
    if (!M.ok) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_ch_classify, blocks_for(n), dim3(256), 0, st, n, (const int32_t *)T.label, (const int *)T.csize, (const int *)T.copen,
                       RSM_MESH_CLOSE_MAX_HOLE, elig, T.ctr);
    hipLaunchKernelGGL(k_ch_sizes, blocks_for(n), dim3(256), 0, st, n, (const int32_t *)T.label, (const int *)T.csize, (const int *)T.copen, d_size);
    DEVCHK(hipMemcpyAsync(d_label, T.label, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    u64 h[H_N];
    DEVCHK(hipMemcpyAsync(h, T.ctr, sizeof h, hipMemcpyDeviceToHost, st));
    if ((s = mesh_finish(st)) != RSM_OK) return s;
    *n_components = (int64_t)h[H_COMPS];
    return RSM_OK;
}

int hole_triangulate_device(const float *d_ring, int L, const uint8_t *d_mask, double *weight, int32_t *d_tri, int *n_tri, hipStream_t st) {
    DevMem M;
    Loops T; // (mesh mode's tables: not read in stage mode)
    unsigned int *nadd = M.get<unsigned int>(1);
    double *w = M.get<double>(1);
    if (!M.ok) return RSM_E_NOMEM;
    launch_fill(L, 1, nullptr, nullptr, T, 0, nullptr, d_ring, d_mask, L, L - 2, d_tri, nadd, w, nullptr, st);
    unsigned int hn = 0;
    DEVCHK(hipMemcpyAsync(&hn, nadd, sizeof hn, hipMemcpyDeviceToHost, st));
    DEVCHK(hipMemcpyAsync(weight, w, sizeof(double), hipMemcpyDeviceToHost, st));
    const int s = mesh_finish(st);
    if (s != RSM_OK) return s;
    *n_tri = (int)hn;
    return RSM_OK;
}

int mesh_close_holes_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const rsm_mesh_close_params *p, PoissonMesh *out, double *stats,
                            int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_, n = 3 * nf;
    double S[RSM_MESH_CLOSE_STATS] = {0};
    S[0] = (double)nv;
    S[1] = (double)nf;
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK) return s;
    DevMem M;
    Loops T;
    PoissonMesh res;
    u64 h[H_N] = {0};
    uint64_t holes = 0, added = 0;
    unsigned int *nadd = nullptr, *off = nullptr;
    int32_t *tri = nullptr;
    int stride = 1;
    const bool work = nv > 0 && nf > 0;
    if (work) {
        if ((s = border_loops(M, T, d_f, nv, nf, st)) != RSM_OK) return s;
        unsigned int *elig = M.get<unsigned int>(n), *epos = M.get<unsigned int>(n);
        if (!M.ok) return RSM_E_NOMEM;
        hipLaunchKernelGGL(k_ch_classify, blocks_for(n), dim3(256), 0, st, n, (const int32_t *)T.label, (const int *)T.csize, (const int *)T.copen, p->max_hole_size, elig,
                           T.ctr);
        if ((s = scan_u32(M, (const unsigned int *)elig, epos, n, st)) != RSM_OK) return s;
        DEVCHK(hipMemcpyAsync(h, T.ctr, sizeof h, hipMemcpyDeviceToHost, st)); // (the longest eligible loop, with the total's round trip)
        if ((s = scan_total(elig, epos, n, st, &holes)) != RSM_OK) return s;
        const int lmax = (int)h[H_LMAX_ELIGIBLE];
        if (holes > 0 && (lmax < 3 || lmax > RSM_MESH_CLOSE_MAX_HOLE)) return RSM_E_HIP; // (cannot be: the classification bounds it)
        if (holes > 0) {
            stride = lmax - 2;
            int *hole = M.get<int>(holes);
            nadd = M.get<unsigned int>(holes);
            off = M.get<unsigned int>(holes);
            tri = M.get<int32_t>(3 * (size_t)stride * holes);
            if (!M.ok) return RSM_E_NOMEM;
            hipLaunchKernelGGL(k_ch_list, blocks_for(n), dim3(256), 0, st, n, (const unsigned int *)elig, (const unsigned int *)epos, hole);
            launch_fill(lmax, holes, d_v, d_f, T, n, hole, nullptr, nullptr, 0, stride, tri, nadd, nullptr, T.ctr, st);
            if ((s = scan_u32(M, (const unsigned int *)nadd, off, holes, st)) != RSM_OK || (s = scan_total(nadd, off, holes, st, &added)) != RSM_OK) return s;
        }
    }
    // the result: the input's vertices and faces, the new faces behind them
    const size_t nfo = nf + (size_t)added;
    if ((s = mesh_result_alloc(res, nv, nfo)) != RSM_OK) return s;
    bool ok = true;
    if (nv > 0) ok = ok && hipMemcpyAsync(res.d_v, d_v, nv * 3 * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (nf > 0) ok = ok && hipMemcpyAsync(res.d_f, d_f, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (added > 0)
        hipLaunchKernelGGL(k_ch_gather, blocks_for((size_t)stride * holes), dim3(256), 0, st, (size_t)stride * holes, stride, (const unsigned int *)nadd,
                           (const unsigned int *)off, (const int32_t *)tri, res.d_f + n);
    if (work) ok = ok && hipMemcpyAsync(h, T.ctr, sizeof h, hipMemcpyDeviceToHost, st) == hipSuccess;
    if (!ok || mesh_finish(st) != RSM_OK) {
        poisson_mesh_free(&res);
        return RSM_E_HIP;
    }
    S[2] = (double)nfo;
    S[3] = (double)h[H_BORDER];
    S[4] = (double)h[H_COMPS];
    S[5] = (double)h[H_LOOPS];
    S[6] = (double)h[H_OPEN];
    S[7] = (double)h[H_CLOSED];
    S[8] = (double)h[H_LONG];
    S[9] = (double)h[H_LONE];
    S[10] = (double)h[H_NOTRI];
    S[11] = (double)added;
    S[12] = (double)h[H_LMAX_CLOSED];
    S[13] = (double)h[H_LMAX_SEEN];
    if (stats) memcpy(stats, S, sizeof S);
    mesh_result_commit(out, res);
    return RSM_OK;
}
