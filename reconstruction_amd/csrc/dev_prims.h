// dev_prims.h -- the host plumbing the cloud units (cloud_grid.hip, k_filter*.hip, k_mls.hip, k_dedup.hip) and the mesh units (k_poisson.hip,
// k_meshclean.hip, k_meshcolor.hip, k_meshstitch.hip) share: the error check, the grid of a thread-per-element launch, rocprim's scan and
// sort with their temporary taken from the caller's allocator, the read-back of a compaction's total, the order-preserving map between
// float and unsigned int behind the exact bounding boxes, and the kernels that renumber a mesh's kept faces and vertices.
// An allocator is anything with get<T>(n) that returns nullptr when it is full: FilterArena (cloud_arena.h), DevMem (mesh_common.h).
#pragma once

#include "../../include/rsm.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h> // (rocprim calls memset without including it)

#include <rocprim/rocprim.hpp>

#define DEVCHK(call)                                \
    do {                                            \
        if ((call) != hipSuccess) return RSM_E_HIP; \
    } while (0)

static inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

static inline int key_bits(unsigned long long x) { // the bits keys 0 .. x use
    int b = 1;
    while (b < 64 && (x >> b) != 0) b++;
    return b;
}

// a scan's temporary, kept by a caller that scans again (the same length or shorter) before it rewinds its allocator
struct ScanTmp {
    void *p = nullptr;
    size_t bytes = 0;
};
// out = the exclusive sums of in[0 .. n); keep (optional): takes the temporary of *keep when it has one, else leaves its own there
template <class Alloc, class In>
static int scan_u32(Alloc &M, In in, unsigned int *out, size_t n, hipStream_t st, ScanTmp *keep = nullptr) {
    ScanTmp t;
    if (keep && keep->p) {
        t = *keep;
    } else {
        DEVCHK(rocprim::exclusive_scan(nullptr, t.bytes, in, out, 0u, n, rocprim::plus<unsigned int>(), st));
        t.p = M.template get<uint8_t>(t.bytes);
        if (!t.p) return RSM_E_NOMEM;
        if (keep) *keep = t;
    }
    DEVCHK(rocprim::exclusive_scan(t.p, t.bytes, in, out, 0u, n, rocprim::plus<unsigned int>(), st));
    return RSM_OK;
}
// (k0, v0) sorted by the low `bits` bits of the keys into (k1, v1), stable
template <class Alloc, typename K>
static int sort_pairs(Alloc &M, K *k0, K *k1, uint32_t *v0, uint32_t *v1, size_t n, int bits, hipStream_t st) {
    size_t tb = 0;
    DEVCHK(rocprim::radix_sort_pairs(nullptr, tb, k0, k1, v0, v1, n, 0, bits, st));
    void *tp = M.template get<uint8_t>(tb);
    if (!tp) return RSM_E_NOMEM;
    DEVCHK(rocprim::radix_sort_pairs(tp, tb, k0, k1, v0, v1, n, 0, bits, st));
    return RSM_OK;
}

// total of a flag (or count) array and its exclusive scan, pos[n - 1] + flag[n - 1]: one host round trip.  h (optional): two words of
// pinned host memory to copy into.
template <typename F>
static int scan_total(const F *flag, const unsigned int *pos, size_t n, hipStream_t st, uint64_t *total, unsigned int *h = nullptr) {
    static_assert(sizeof(F) <= sizeof(unsigned int), "a flag fits a word");
    unsigned int own[2];
    if (!h) h = own;
    h[0] = h[1] = 0u;
    DEVCHK(hipMemcpyAsync(&h[0], pos + (n - 1), sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    DEVCHK(hipMemcpyAsync(&h[1], flag + (n - 1), sizeof(F), hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    *total = (uint64_t)h[0] + (uint64_t)h[1];
    return RSM_OK;
}
// ... of two arrays in one round trip
static inline int scan_totals(const unsigned int *flag_a, const unsigned int *pos_a, size_t na, const unsigned int *flag_b, const unsigned int *pos_b, size_t nb,
                              hipStream_t st, uint64_t *total_a, uint64_t *total_b) {
    unsigned int h[4] = {0, 0, 0, 0};
    DEVCHK(hipMemcpyAsync(h, pos_a + (na - 1), sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    DEVCHK(hipMemcpyAsync(h + 1, flag_a + (na - 1), sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    DEVCHK(hipMemcpyAsync(h + 2, pos_b + (nb - 1), sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    DEVCHK(hipMemcpyAsync(h + 3, flag_b + (nb - 1), sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    *total_a = (uint64_t)h[0] + h[1];
    *total_b = (uint64_t)h[2] + h[3];
    return RSM_OK;
}

// order-preserving map float -> uint (atomicMin / atomicMax on it give the exact float min / max) and back.  (The way back is an xor and
// not a select of two forms: hipcc 7.2's instruction selection fails on the select inside a kernel.)
__host__ __device__ __forceinline__ unsigned int f2ord(float f) {
    unsigned int u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float ord2f(unsigned int u) {
    const unsigned int v = u ^ ((u >> 31) ? 0x80000000u : 0xffffffffu);
    float f;
    __builtin_memcpy(&f, &v, 4);
    return f;
}

// the kept faces / the used vertices of a mesh, renumbered in order (fpos / vpos: the exclusive scans of fkeep / vused).  Templates: the
// units are compiled without relocatable device code, and only a unit that launches them (k_mesh_compact_faces<>) holds a copy
template <int = 0>
__global__ __launch_bounds__(256) void k_mesh_compact_faces(const int32_t *__restrict__ faces, size_t nf, const unsigned int *__restrict__ fkeep,
                                                            const unsigned int *__restrict__ fpos, const unsigned int *__restrict__ vpos,
                                                            int32_t *__restrict__ out) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf || !fkeep[f]) return;
    const size_t o = fpos[f];
    for (int c = 0; c < 3; c++) out[3 * o + c] = (int32_t)vpos[faces[3 * f + c]];
}
template <int = 0>
__global__ __launch_bounds__(256) void k_mesh_compact_verts(const float *__restrict__ verts, size_t nv, const unsigned int *__restrict__ vused,
                                                            const unsigned int *__restrict__ vpos, float *__restrict__ out) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv || !vused[v]) return;
    const size_t o = vpos[v];
    for (int c = 0; c < 3; c++) out[3 * o + c] = verts[3 * v + c];
}
