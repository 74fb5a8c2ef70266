// subdivide_limits.h -- whether the mesh one iteration of the Loop subdivision (k_meshsubdivide.hip) is about to make still
// fits the mesh layer's indices: the one copy of that check, for the stage (which asks it with the counted totals, before it allocates the
// iteration's result) and for the program that holds it against 128-bit arithmetic at the boundaries (tests/cpp/subdivide_limits_check.cpp,
// plain g++).
//
// The layer's limits (rsm_mesh.hip's mesh_counts_ok): a vertex index is an int32, so nv <= INT32_MAX; the edge table and the corner lists
// number their entries 3 f + j in 31 bits, so 3 nf < 2^31.  An iteration that splits n_split edges of a mesh of nv_in vertices leaves
// nv_in + n_split vertices and nf_out faces (every face replaced by 1..4).  Nothing here multiplies or adds what could wrap: the arguments
// are any uint64.
#ifndef RSM_SUBDIVIDE_LIMITS_H
#define RSM_SUBDIVIDE_LIMITS_H

#include <stdint.h>

#define SUBDIVIDE_MAX_VERTICES ((uint64_t)INT32_MAX)
#define SUBDIVIDE_MAX_FACES ((((uint64_t)1 << 31) - 1) / 3) /* the largest nf with 3 nf < 2^31: 715827882 */

// 1: nv_in + n_split <= INT32_MAX and 3 nf_out < 2^31; 0: the iteration's result would be too large
static inline int subdivide_sizes_ok(uint64_t nv_in, uint64_t n_split, uint64_t nf_out) {
    if (nv_in > SUBDIVIDE_MAX_VERTICES || n_split > SUBDIVIDE_MAX_VERTICES - nv_in) return 0;
    return nf_out <= SUBDIVIDE_MAX_FACES ? 1 : 0;
}

#endif
