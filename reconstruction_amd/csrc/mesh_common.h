// mesh_common.h -- what the surface (k_poisson.hip), its smoothing / clean-up (k_meshclean.hip) and its density trim (k_meshtrim.hip) share
// beyond dev_prims.h: the scratch of one call, the mesh tables the colouring reads as well, the edge keys and the union-find.
#pragma once

#include "dev_prims.h"

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

// what k_meshclean.hip builds and the colouring (k_meshcolor.hip) reads as well.  validate: RSM_OK, or RSM_E_INVALID with *invalid = 1 (a
// face index outside [0, nv)) / 2 (a coordinate that is not finite); d_v may be NULL (indices only).  corner lists: a CSR over the vertices
// of the corners 3 f + j that hold them, each list ascending (row: nv + 1 starts, corner: 3 nf entries, both M's); faces with a repeated
// index are in no list.
int mesh_validate_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, int *invalid, hipStream_t st);
int mesh_corner_lists_device(DevMem &M, const int32_t *d_f, size_t nv, size_t nf, uint32_t **row, uint32_t **corner, hipStream_t st);

// ---- the sorted edge table's keys and the union-find over it (k_meshclean.hip, k_meshtrim.hip) ---------------------------------------------
__device__ __forceinline__ bool face_distinct(int a, int b, int c) { return a != b && b != c && a != c; }

// entry 3 f + j: key (min << 32) | max of edge j = (v_j, v_j+1); a face with a repeated index gets the key after every edge, nv << 32.
// (Templates for the reason dev_prims.h gives: only a unit that launches them holds a copy.)
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
