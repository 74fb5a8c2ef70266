// poisson_common.h -- what the dense-grid Poisson surface (k_poisson.hip) and its banded finest level (k_poisson_band.hip) share beyond
// rsm_dev.h: the fixed-point scale of the splat, the grid of a call, the marching-tetrahedra tables (the lattice edge directions, the six
// Kuhn tetrahedra, the 16 cases) and the trim's face rule.  The kernel is a template for the reason dev_prims.h gives.
#pragma once

#include "mesh_common.h"
#include "rsm_dev.h"

#include <string.h>

#define PV_FIX 4294967296.0 // 2^32: the splat's fixed-point scale

struct PvGrid {
    double ox, oy, oz, h;
    int sh, N; // N = 1 << sh
};

// the 16 cases of a tetrahedron (v0..v3, bit i of the case = v_i inside), for a positively oriented tetrahedron: faces as edges (u, v), u < v,
// wound so that the normal points to the outside vertices; a negatively oriented tetrahedron swaps the last two corners of each face
struct TetTable {
    uint8_t ntri[16];
    uint8_t e[16][2][3]; // edge code u << 2 | v
};

// ---- 7: marching tetrahedra: the tables -------------------------------------------------------------------------------------------
// direction codes of a lattice edge (a, b = a + d): 100, 010, 001, 110, 101, 011, 111 (x, y, z)
static __device__ __constant__ int8_t c_dir[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
__device__ __forceinline__ int pv_dir_code(int dx, int dy, int dz) { // offsets in {0, 1}, not all 0
    const int m = dx | (dy << 1) | (dz << 2); // 1..7
    // m: 1 -> 0 (100), 2 -> 1 (010), 4 -> 2 (001), 3 -> 3 (110), 5 -> 4 (101), 6 -> 5 (011), 7 -> 6
    return (0x6542310 >> (4 * (m - 1))) & 7;
}
// the axis permutations (a, b, c) in lexicographic order; tetrahedron = 000, +a, +a+b, 111; its orientation is the permutation's sign
static __device__ __constant__ int8_t c_perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
static __device__ __constant__ int8_t c_perm_sign[6] = {1, -1, -1, 1, 1, -1};

// ---- 8: trim: the face rule ----------------------------------------------------------------------------------------------------------
template <int = 0>
__global__ __launch_bounds__(256) void k_pv_face_keep(const int32_t *__restrict__ faces, size_t nf, const uint8_t *__restrict__ vkeep,
                                                      unsigned int *__restrict__ fkeep, unsigned int *__restrict__ vused) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nf) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const unsigned int keep = (vkeep[a] && vkeep[b] && vkeep[c] && a != b && b != c && a != c) ? 1u : 0u;
    fkeep[f] = keep;
    if (keep) vused[a] = vused[b] = vused[c] = 1u; // (every writer stores the same value)
}

static inline TetTable make_tet_table() {
    TetTable T;
    memset(&T, 0, sizeof T);
    auto edge = [](int u, int v) { return (uint8_t)(u < v ? (u << 2 | v) : (v << 2 | u)); };
    for (int m = 1; m < 15; m++) {
        int in[4], ni = 0, out[4], no = 0;
        for (int v = 0; v < 4; v++) {
            if ((m >> v) & 1) in[ni++] = v;
            else out[no++] = v;
        }
        if (ni == 1 || ni == 3) {
            const int L = ni == 1 ? in[0] : out[0];
            const int *o = ni == 1 ? out : in; // the three others, ascending
            // (L, A, B, C) is an even permutation of (0, 1, 2, 3) iff L is even: the face (LA, LB, LC) then looks away from L
            const bool away = (L & 1) == 0;
            const bool want_away = ni == 1; // L inside: the outside is away from it
            T.ntri[m] = 1;
            T.e[m][0][0] = edge(L, o[0]);
            T.e[m][0][1] = edge(L, away == want_away ? o[1] : o[2]);
            T.e[m][0][2] = edge(L, away == want_away ? o[2] : o[1]);
        } else {
            const int P = in[0], Q = in[1], R = out[0], S = out[1];
            const int perm[4] = {P, Q, R, S};
            int inv = 0;
            for (int a = 0; a < 4; a++)
                for (int b = a + 1; b < 4; b++) inv += perm[a] > perm[b];
            const bool even = (inv & 1) == 0; // (P, Q, R, S) positively oriented: the quad PR, PS, QS, QR looks toward R, S
            const uint8_t pr = edge(P, R), ps = edge(P, S), qs = edge(Q, S), qr = edge(Q, R);
            T.ntri[m] = 2;
            T.e[m][0][0] = pr; T.e[m][0][1] = even ? ps : qs; T.e[m][0][2] = even ? qs : ps;
            T.e[m][1][0] = pr; T.e[m][1][1] = even ? qs : qr; T.e[m][1][2] = even ? qr : qs;
        }
    }
    return T;
}


// (k_poisson.hip) step 8's second half: of `full`, whose vertices vkeep flags, the faces whose three vertices are kept and distinct, the
// vertices they use, both renumbered in order -> *out (mesh_result_commit); `full` is freed.  M: the call's scratch
int poisson_trim_commit(DevMem &M, PoissonMesh &full, const uint8_t *vkeep, PoissonMesh *out, hipStream_t st);
