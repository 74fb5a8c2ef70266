// mesh_common.h -- the mesh units' topology layer, beyond dev_prims.h: what the surface (k_poisson.hip), its smoothing / clean-up
// (k_meshclean.hip), its density trim (k_meshtrim.hip), the closing of its holes (k_meshclose.hip), its decimation (k_meshdecimate.hip), its subdivision
// (k_meshsubdivide.hip) and its colours (k_meshcolor.hip, k_meshstitch.hip, k_meshfill.hip) share.  The scratch of one call; the sorted edge table and the corner lists of a mesh,
// built from any allocator (dev_prims.h: DevMem and Pool here); the neighbour CSR over the corner lists; the Chebyshev schedule; the union-find over the table; the vertex box and its
// diagonal; a point in fp64; the end of a call that replaces a mesh.  What a stage does with the table's runs stays in its own unit.
// The kernels are templates for the reason dev_prims.h gives: only a unit that launches one (k_mesh_edge_keys<>) holds a copy.
#pragma once

#include "dev_prims.h"
#include "rsm_dev.h"

#include <algorithm>
#include <vector>

struct DevMem { // scratch of one call
    std::vector<void *> p;
    bool ok = true;
    template <typename T> T *get(size_t n) {
        void *q = nullptr;
        if (!ok || hipMalloc(&q, (n ? n : 1) * sizeof(T)) != hipSuccess) {
            ok = false;
            return nullptr;
        }
        p.push_back(q);
        return (T *)q;
    }
    ~DevMem() {
        for (void *q : p) (void)hipFree(q);
    }
};

// the scratch of a stage that runs rounds: an allocator (dev_prims.h) that hands out pieces of a few large blocks and starts over with
// rewind(), so that only the first round allocates (the decimation: a later round asks for the same pieces in the same order, none of them
// larger); without rewind() it is one hipMalloc for everything that fits its first block (the subdivision: a pool an iteration)
struct Pool {
    struct Block {
        uint8_t *p;
        size_t size;
    };
    std::vector<Block> blocks;
    size_t cur = 0, off = 0, first;
    explicit Pool(size_t first_block) : first(first_block) {}
    ~Pool() {
        for (Block &b : blocks) (void)hipFree(b.p);
    }
    void rewind() { cur = off = 0; }
    template <typename T> T *get(size_t n) {
        const size_t bytes = (((n ? n : 1) * sizeof(T)) + 255) & ~(size_t)255;
        for (;; cur++, off = 0) {
            if (cur == blocks.size()) {
                void *q = nullptr;
                const size_t size = std::max(bytes, first);
                if (hipMalloc(&q, size) != hipSuccess) return nullptr;
                blocks.push_back(Block{(uint8_t *)q, size});
            }
            if (off + bytes <= blocks[cur].size) {
                T *r = (T *)(blocks[cur].p + off);
                off += bytes;
                return r;
            }
        }
    }
};

// (k_meshclean.hip) RSM_OK, or RSM_E_INVALID with *invalid = 1 (a face index outside [0, nv)) / 2 (a coordinate that is not finite); d_v may
// be NULL (indices only)
int mesh_validate_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, int *invalid, hipStream_t st);

// (k_meshtrim.hip) f11's items 2 and 3 on f7's box grid = {o, h of 2^depth nodes}, h > 0: the count splat of the n samples on 2^kernel_depth
// nodes per axis, read back at nv points (float xyz) -> d_rho (may be NULL), d_val.  Enqueues only; its scratch is M's
int density_at_points_device(DevMem &M, const float *d_sx, const float *d_sn4, int64_t n, int depth, const double grid[4], int kernel_depth,
                             double samples_per_node, const float *d_v, int64_t nv, double *d_rho, double *d_val, hipStream_t st);

static inline int mesh_finish(hipStream_t st) {
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    return RSM_OK;
}

// a vertex in fp64
struct D3 {
    double x, y, z;
};
__device__ __forceinline__ D3 ld3(const float *__restrict__ v, size_t i) { return D3{(double)v[3 * i], (double)v[3 * i + 1], (double)v[3 * i + 2]}; }

// ---- the sorted edge table and the union-find over it ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool face_distinct(int a, int b, int c) { return a != b && b != c && a != c; }

// entry 3 f + j: key (min << 32) | max of edge j = (v_j, v_j+1); a face with a repeated index gets the key after every edge, nv << 32
template <int = 0>
__global__ __launch_bounds__(256) void k_mesh_edge_keys(const int32_t *__restrict__ f, size_t nf, unsigned long long nv, unsigned long long *__restrict__ key,
                                                        uint32_t *__restrict__ val) {
    typedef unsigned long long u64;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const int v[3] = {f[3 * i], f[3 * i + 1], f[3 * i + 2]};
    const bool ok = face_distinct(v[0], v[1], v[2]);
    for (int j = 0; j < 3; j++) {
        const u64 a = (u64)v[j], b = (u64)v[(j + 1) % 3];
        key[3 * i + j] = ok ? ((a < b ? a : b) << 32 | (a < b ? b : a)) : nv << 32;
        val[3 * i + j] = (uint32_t)(3 * i + j);
    }
}
template <int = 0>
__global__ __launch_bounds__(256) void k_mesh_iota(int *__restrict__ a, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = (int)i;
}

// the table of nf > 0 faces: (ekey, eval) = the 3 nf keys and their entries 3 f + j, sorted by rocprim's stable radix sort over the key bits
// in use; (k0, v0) = the unsorted ones.  A run of equal keys = the faces on one edge; the faces of a run ascend.  The four buffers (3 nf
// each) are the caller's, allocated where it allocates its own: a stage allocates everything before it enqueues anything, and a
// hipMalloc issued once work is on the stream costs the call time (profiles/LAB_NOTES.md, f23); only the sort's temporary comes from M here.
template <class Alloc>
static int mesh_edge_table(Alloc &M, const int32_t *d_f, size_t nv, size_t nf, unsigned long long *k0, uint32_t *v0, unsigned long long *ekey, uint32_t *eval,
                           hipStream_t st) {
    typedef unsigned long long u64;
    hipLaunchKernelGGL(k_mesh_edge_keys<>, blocks_for(nf), dim3(256), 0, st, d_f, nf, (u64)nv, k0, v0);
    return sort_pairs(M, k0, ekey, v0, eval, 3 * nf, 32 + key_bits((u64)nv), st);
}

__device__ __forceinline__ int uf_load(int *parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the root of x; halves the path on the way (a parent only ever moves to an ancestor, and ancestors have lower indices)
__device__ __forceinline__ int uf_find(int *parent, int x) {
    int p = uf_load(parent, x);
    while (p != x) {
        const int g = uf_load(parent, p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}
// the larger root hooks under the smaller, so every root is the lowest index of its tree whatever the order of the hooks
__device__ __forceinline__ void uf_union(int *parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(parent + b, b, a) == b) return; // (b was still a root; otherwise somebody hooked it first: again)
    }
}

// ---- the corner lists: a CSR over the vertices of the corners 3 f + j that hold them, each list ascending -------------------------------------
// key = the vertex of corner 3 f + j, nv for the corners of a face with a repeated index (they sort behind every list)
template <int = 0>
__global__ __launch_bounds__(256) void k_mesh_corner_keys(const int32_t *__restrict__ f, size_t nf, uint32_t nv, uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const int v[3] = {f[3 * i], f[3 * i + 1], f[3 * i + 2]};
    const bool ok = face_distinct(v[0], v[1], v[2]);
    for (int j = 0; j < 3; j++) {
        key[3 * i + j] = ok ? (uint32_t)v[j] : nv;
        val[3 * i + j] = (uint32_t)(3 * i + j);
    }
}
// row[v] = the first sorted position whose key is >= v, v = 0 .. nv
template <int = 0>
__global__ __launch_bounds__(256) void k_mesh_row_starts(const uint32_t *__restrict__ key, size_t n, size_t nv, uint32_t *__restrict__ row) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v > nv) return;
    size_t lo = 0, hi = n;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (key[mid] < (uint32_t)v) lo = mid + 1;
        else hi = mid;
    }
    row[v] = (uint32_t)lo;
}
// row: nv + 1 starts, corner: 3 nf entries, both M's; faces with a repeated index are in no list.  nf = 0: every start is 0.
template <class Alloc>
static int mesh_corner_lists(Alloc &M, const int32_t *d_f, size_t nv, size_t nf, uint32_t **row, uint32_t **corner, hipStream_t st) {
    const size_t n = 3 * nf;
    uint32_t *k0 = M.template get<uint32_t>(n), *k1 = M.template get<uint32_t>(n), *v0 = M.template get<uint32_t>(n);
    *corner = M.template get<uint32_t>(n);
    *row = M.template get<uint32_t>(nv + 1);
    if (!k0 || !k1 || !v0 || !*corner || !*row) return RSM_E_NOMEM;
    if (nf > 0) {
        hipLaunchKernelGGL(k_mesh_corner_keys<>, blocks_for(nf), dim3(256), 0, st, d_f, nf, (uint32_t)nv, k0, v0);
        const int s = sort_pairs(M, k0, k1, v0, *corner, n, key_bits((unsigned long long)nv), st);
        if (s != RSM_OK) return s;
    }
    hipLaunchKernelGGL(k_mesh_row_starts<>, blocks_for(nv + 1), dim3(256), 0, st, (const uint32_t *)k1, n, nv, *row);
    return RSM_OK;
}

// ---- the neighbour CSR over the corner lists (k_meshtrim.hip's value smoothing, k_meshfill.hip) -----------------------------------------------
// row i starts at 2 row[i] (a corner gives two: f[(j+1)%3] then f[(j+2)%3]) and holds 2 (row[i + 1] - row[i]) entries: every neighbour,
// an interior edge twice, a border edge once
template <int = 0>
__global__ __launch_bounds__(256) void k_mesh_nbr_csr(size_t nv, const int32_t *__restrict__ f, const uint32_t *__restrict__ row, const uint32_t *__restrict__ corner,
                                                      uint32_t *__restrict__ nbr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    for (uint32_t r = row[i]; r < row[i + 1]; r++) {
        const uint32_t c = corner[r];
        const size_t fi = c / 3;
        const uint32_t j = c % 3;
        nbr[2 * (size_t)r] = (uint32_t)f[3 * fi + (j + 1) % 3];
        nbr[2 * (size_t)r + 1] = (uint32_t)f[3 * fi + (j + 2) % 3];
    }
}

// ---- the Chebyshev iteration's schedule on the host (k_meshstitch.hip, k_meshfill.hip) ---------------------------------------
// the eigenvalues of the Jacobi-preconditioned matrix lie in [lmin, 2]; step k = 0, 1, ... in order: d = alpha d + beta z
struct ChebSchedule {
    double theta, delta, sigma, rho;
    explicit ChebSchedule(double lmin) : theta((2.0 + lmin) / 2.0), delta((2.0 - lmin) / 2.0) {
        sigma = theta / delta;
        rho = 1.0 / sigma;
    }
    void step(int k, double *alpha, double *beta) {
        *alpha = 0.0;
        *beta = 1.0 / theta;
        if (k >= 1) {
            const double rn = 1.0 / (2.0 * sigma - rho);
            *alpha = rn * rho;
            *beta = (2.0 * rn) / delta;
            rho = rn;
        }
    }
};
// the least k >= 1 with T_k(sigma) >= 1 / reduction, T_k+1 = 2 sigma T_k - T_k-1; -1: more than max_steps
static inline int cheb_steps(double lmin, double reduction, int max_steps) {
    const double sigma = ChebSchedule(lmin).sigma;
    const double target = 1.0 / reduction;
    double t0 = 1.0, t1 = sigma;
    int k = 1;
    while (t1 < target) {
        if (k == max_steps) return -1;
        const double t2 = (2.0 * sigma) * t1 - t0;
        t0 = t1;
        t1 = t2;
        k++;
    }
    return k;
}

// ---- the box of the vertices: mm[0 .. 5] = min x, y, z, max x, y, z as ordered uints (dev_prims.h), preset to ~0 / 0 ---------------------------
template <int = 0>
__global__ __launch_bounds__(256) void k_mesh_vertex_box(const float *__restrict__ p, size_t nv, unsigned int *__restrict__ mm) {
    __shared__ unsigned int s_mm[6];
    if (threadIdx.x < 6) s_mm[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (size_t)gridDim.x * 256)
        for (int a = 0; a < 3; a++) {
            const unsigned int o = f2ord(p[3 * v + a]);
            atomicMin(&s_mm[a], o);
            atomicMax(&s_mm[3 + a], o);
        }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&mm[threadIdx.x], s_mm[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&mm[threadIdx.x], s_mm[threadIdx.x]);
}
// the square of such a box's fp64 diagonal
__host__ __device__ __forceinline__ double box_diagonal2(const unsigned int *b) {
    const double dx = (double)ord2f(b[3]) - (double)ord2f(b[0]), dy = (double)ord2f(b[4]) - (double)ord2f(b[1]), dz = (double)ord2f(b[5]) - (double)ord2f(b[2]);
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- the end of a call that replaces a mesh ---------------------------------------------------------------------------------------------------
// res = room for kv vertices and kf faces (a count of 0 gets no buffer); when either allocation fails res is freed whole
static inline int mesh_result_alloc(PoissonMesh &res, size_t kv, size_t kf) {
    if ((kv > 0 && hipMalloc((void **)&res.d_v, kv * 3 * sizeof(float)) != hipSuccess) || (kf > 0 && hipMalloc((void **)&res.d_f, kf * 3 * sizeof(int32_t)) != hipSuccess)) {
        poisson_mesh_free(&res);
        return RSM_E_NOMEM;
    }
    res.nv = (int64_t)kv;
    res.nf = (int64_t)kf;
    return RSM_OK;
}
// *out may own the buffers the call read: it goes only now, after the last read
static inline void mesh_result_commit(PoissonMesh *out, const PoissonMesh &res) {
    poisson_mesh_free(out);
    *out = res;
}

// ---- f7's valid sample (k_poisson.hip, k_meshtrim.hip): finite point and normal, normal != 0; p = the point, nh = the unit normal, fp64 ------
__device__ __forceinline__ bool pv_valid(const float *__restrict__ xyz, const float *__restrict__ nrm, int64_t s, double p[3], double nh[3]) {
    const float x = xyz[3 * s], y = xyz[3 * s + 1], z = xyz[3 * s + 2];
    const float a = nrm[4 * s], b = nrm[4 * s + 1], c = nrm[4 * s + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z) && isfinite(a) && isfinite(b) && isfinite(c))) return false;
    const double da = (double)a, db = (double)b, dc = (double)c;
    const double nn = (da * da + db * db) + dc * dc;
    if (!(nn > 0.0)) return false;
    const double len = sqrt(nn);
    nh[0] = da / len; nh[1] = db / len; nh[2] = dc / len;
    p[0] = (double)x; p[1] = (double)y; p[2] = (double)z;
    return true;
}
// ... without normals (the density trim's samples may come without): a finite point
__device__ __forceinline__ bool pv_valid_point(const float *__restrict__ xyz, int64_t s, double p[3]) {
    const float x = xyz[3 * s], y = xyz[3 * s + 1], z = xyz[3 * s + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    p[0] = (double)x; p[1] = (double)y; p[2] = (double)z;
    return true;
}

// ---- f7's trilinear cell on a cubic grid of N nodes per axis at o + (i + 1/2) h (k_meshtrim.hip, k_poisson_density.hip) ------------------------
struct MtGrid {
    double ox, oy, oz, h;
    int N;
};
// the first node per axis and the fraction toward the next
__device__ __forceinline__ void mt_cell(const double p[3], const MtGrid &g, double fl[3], double f[3]) {
    const double o[3] = {g.ox, g.oy, g.oz};
    for (int a = 0; a < 3; a++) {
        const double gq = (p[a] - o[a]) / g.h - 0.5;
        fl[a] = floor(gq);
        f[a] = gq - fl[a];
    }
}
__device__ __forceinline__ double mt_weight(const double f[3], int dx, int dy, int dz) {
    return ((dx ? f[0] : 1.0 - f[0]) * (dy ? f[1] : 1.0 - f[1])) * (dz ? f[2] : 1.0 - f[2]);
}
// fl as node indices when the cell touches the grid (fl in [-1, N - 1]; the test keeps a cast of anything else, NaN included, out)
__device__ __forceinline__ bool mt_cell_index(const double fl[3], int N, int i0[3]) {
    if (!(fl[0] >= -1.0 && fl[1] >= -1.0 && fl[2] >= -1.0 && fl[0] < (double)N && fl[1] < (double)N && fl[2] < (double)N)) return false;
    i0[0] = (int)fl[0]; i0[1] = (int)fl[1]; i0[2] = (int)fl[2];
    return true;
}
