// mesh_common.h -- what the surface (k_poisson.hip) and its smoothing / clean-up (k_meshclean.hip) share: the scratch of one call, the
// grid of a thread-per-element launch, and the order-preserving map between float and unsigned int behind the exact bounding boxes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

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

static inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

// what k_meshclean.hip builds and the colouring (k_meshcolor.hip) reads as well.  validate: RSM_OK, or RSM_E_INVALID with *invalid = 1 (a
// face index outside [0, nv)) / 2 (a coordinate that is not finite); d_v may be NULL (indices only).  corner lists: a CSR over the vertices
// of the corners 3 f + j that hold them, each list ascending (row: nv + 1 starts, corner: 3 nf entries, both M's); faces with a repeated
// index are in no list.
int mesh_validate_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, int *invalid, hipStream_t st);
int mesh_corner_lists_device(DevMem &M, const int32_t *d_f, size_t nv, size_t nf, uint32_t **row, uint32_t **corner, hipStream_t st);

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
