// poisson_band_common.h -- what the units that work on a band of bricks share (k_poisson_band.hip, k_poisson_band_density.hip):
// the band as a kernel sees it and the way from a node to its element.  Fields are brick-major: element slot * 512 + lx + 8 (ly + 8 lz).
#pragma once

#include "poisson_common.h"
#include "rsm_dev.h"

#define PB_NODES 512 // nodes of a brick

struct PbBand { // what a kernel needs of a PoissonBand
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

static inline PvGrid pb_grid(const double grid[4], int depth) { return PvGrid{grid[0], grid[1], grid[2], grid[3], depth, 1 << depth}; }
static inline PbBand pb_band(const PoissonBand &b) { return PbBand{b.d_slot, b.d_active, b.d_nbr, b.depth, b.depth - 3, 1 << b.depth}; }
static inline size_t pb_nodes(const PoissonBand &b) { return (size_t)b.n_active * PB_NODES; }
