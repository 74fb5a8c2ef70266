// mesh_common.h -- what the surface (k_poisson.hip) and its smoothing / clean-up (k_meshclean.hip) share beyond dev_prims.h: the scratch
// of one call and the mesh tables the colouring reads as well.
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
