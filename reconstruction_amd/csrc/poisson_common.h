// poisson_common.h -- the extraction of the Poisson surface, stated once over the node space (poisson_space.h):
// the marching-tetrahedra tables (the lattice edge directions, the six Kuhn tetrahedra, the 16 cases), the three kernels (edge flags, vertices,
// faces), the host sequence that runs them on a dense grid (k_poisson.hip) or a band of bricks (k_poisson_band.hip), and the trim's face rule.
// The kernels are templates for the reason dev_prims.h gives.
#pragma once

#include "mesh_common.h"
#include "poisson_space.h"
#include "rsm_dev.h"

#include <string.h>

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


// flag8[a]: byte d = the edge (a, d) has both ends in the space and crosses the surface; cnt[a] = how many of them
template <class Space>
__global__ __launch_bounds__(256) void k_pv_edge_flags(const float *__restrict__ chi, float iso, Space S, unsigned long long *__restrict__ flag8,
                                                       unsigned int *__restrict__ cnt) {
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= S.nodes()) return;
    const auto n = S.at(a);
    const bool ia = chi[a] < iso;
    unsigned long long w = 0;
    unsigned int m = 0;
    for (int d = 0; d < 7; d++) {
        const long long e = S.nbr(n, c_dir[d][0], c_dir[d][1], c_dir[d][2]);
        if (e < 0) continue;
        if (ia != (chi[e] < iso)) {
            w |= 1ull << (8 * d);
            m++;
        }
    }
    flag8[a] = w;
    cnt[a] = m;
}
// the vertex of edge (a, d): a's first vertex plus the flagged directions below d (the vertices ascend by (a, d))
__device__ __forceinline__ unsigned int pv_vertex_of_edge(const unsigned long long *__restrict__ flag8, const unsigned int *__restrict__ vpos, size_t a, int d) {
    return vpos[a] + (unsigned int)__popcll(flag8[a] & ((1ull << (8 * d)) - 1ull));
}
// one vertex per flagged edge; vkeep (optional) = its cell lies in the mask
template <class Space>
__global__ __launch_bounds__(256) void k_pv_emit_vertices(const float *__restrict__ chi, float iso, MtGrid g, Space S, const unsigned long long *__restrict__ flag8,
                                                          const unsigned int *__restrict__ vpos, float *__restrict__ verts, const uint8_t *__restrict__ mask,
                                                          uint8_t *__restrict__ vkeep) {
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= S.nodes()) return;
    const unsigned long long w = flag8[a];
    if (w == 0) return;
    const auto n = S.at(a);
    int ijk[3];
    S.coords(n, ijk);
    const double o[3] = {g.ox, g.oy, g.oz};
    const float ca = chi[a];
    size_t v = vpos[a];
    for (int d = 0; d < 7; d++) {
        if (!((w >> (8 * d)) & 1)) continue;
        const float cb = chi[S.nbr(n, c_dir[d][0], c_dir[d][1], c_dir[d][2])];
        const float t = (iso - ca) / (cb - ca);
        int cell[3];
        for (int c = 0; c < 3; c++) {
            const float pa = (float)(o[c] + ((double)ijk[c] + 0.5) * g.h);
            const float pb = (float)(o[c] + ((double)(ijk[c] + c_dir[d][c]) + 0.5) * g.h);
            const float p = pa + t * (pb - pa);
            verts[3 * v + c] = p;
            cell[c] = pv_occ_cell((double)p, o[c], g.h, g.N);
        }
        if (vkeep) {
            const long long e = S.elem(cell[0], cell[1], cell[2]);
            vkeep[v] = e < 0 ? 0 : mask[e];
        }
        v++;
    }
}
// faces of a cell whose eight corners lie in the space (its 000 node is `a`): EMIT = false counts them, true writes them at foff[a] in
// (tetrahedron, triangle) order
template <bool EMIT, class Space>
__global__ __launch_bounds__(256) void k_pv_cell_faces(const float *__restrict__ chi, float iso, Space S, TetTable tab, unsigned int *__restrict__ cnt,
                                                       const unsigned int *__restrict__ foff, const unsigned long long *__restrict__ flag8,
                                                       const unsigned int *__restrict__ vpos, int32_t *__restrict__ faces) {
    const size_t a = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= S.nodes()) return;
    const auto n = S.at(a);
    long long ce[8];
    bool whole = true;
    for (int c = 0; c < 8; c++) {
        ce[c] = S.nbr(n, c & 1, (c >> 1) & 1, (c >> 2) & 1);
        whole = whole && ce[c] >= 0;
    }
    unsigned int cube = 0; // bit (dx | dy << 1 | dz << 2) = that corner is inside
    if (whole)
        for (int c = 0; c < 8; c++)
            if (chi[ce[c]] < iso) cube |= 1u << c;
    if (!whole || cube == 0 || cube == 255) {
        if (!EMIT) cnt[a] = 0;
        return;
    }
    unsigned int nf = 0;
    size_t o = EMIT ? (size_t)foff[a] : 0;
    for (int t = 0; t < 6; t++) {
        const int pa = c_perm[t][0], pb = c_perm[t][1];
        const int corner[4] = {0, 1 << pa, (1 << pa) | (1 << pb), 7};
        int m = 0;
        for (int v = 0; v < 4; v++) m |= ((cube >> corner[v]) & 1) << v;
        const int nt = tab.ntri[m];
        if (!EMIT) {
            nf += nt;
            continue;
        }
        for (int q = 0; q < nt; q++) {
            int32_t vi[3];
            for (int c = 0; c < 3; c++) {
                const int e = tab.e[m][q][c];
                const int cu = corner[e >> 2], cv = corner[e & 3]; // cu is a subset of cv: the lower node is cu's
                const int d = cv & ~cu;
                long long na = ce[0];
                for (int k = 1; k < 8; k++) na = k == cu ? ce[k] : na; // (no dynamic index into ce: it stays in registers)
                vi[c] = (int32_t)pv_vertex_of_edge(flag8, vpos, (size_t)na, pv_dir_code(d & 1, (d >> 1) & 1, (d >> 2) & 1));
            }
            if (c_perm_sign[t] < 0) {
                const int32_t w = vi[1];
                vi[1] = vi[2];
                vi[2] = w;
            }
            faces[3 * o] = vi[0];
            faces[3 * o + 1] = vi[1];
            faces[3 * o + 2] = vi[2];
            o++;
        }
    }
    if (!EMIT) cnt[a] = nf;
}

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

// steps 7 and 8 on a node space: flags -> scan -> faces counted -> scan -> vertices and faces, then (trim_cells > 0 with d_occ) the trim by the
// occupancy that dilate(in, out, axis) widens one axis at a time.  The mesh -> *out; untrimmed = its counts before the trim
template <class Space, class Dilate>
static int poisson_extract(const Space &S, const MtGrid &g, const float *d_chi, double iso, const uint8_t *d_occ, int trim_cells, Dilate dilate, PoissonMesh *out,
                           int64_t untrimmed[2], hipStream_t st) {
    poisson_mesh_free(out);
    untrimmed[0] = untrimmed[1] = 0;
    const size_t nodes = S.nodes();
    if (nodes == 0) return RSM_OK;
    const float iso32 = (float)iso;
    const TetTable tab = make_tet_table();
    const bool trim = trim_cells > 0 && d_occ;
    DevMem M;
    unsigned long long *flag8 = M.get<unsigned long long>(nodes);
    unsigned int *vcnt = M.get<unsigned int>(nodes), *vpos = M.get<unsigned int>(nodes), *cnt = M.get<unsigned int>(nodes), *foff = M.get<unsigned int>(nodes);
    uint8_t *t0 = trim ? M.get<uint8_t>(nodes) : nullptr, *t1 = trim ? M.get<uint8_t>(nodes) : nullptr;
    if (!M.ok) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_pv_edge_flags<Space>, blocks_for(nodes), dim3(256), 0, st, d_chi, iso32, S, flag8, vcnt);
    int s = scan_u32(M, (const unsigned int *)vcnt, vpos, nodes, st);
    if (s != RSM_OK) return s;
    hipLaunchKernelGGL((k_pv_cell_faces<false, Space>), blocks_for(nodes), dim3(256), 0, st, d_chi, iso32, S, tab, cnt, (const unsigned int *)nullptr,
                       (const unsigned long long *)nullptr, (const unsigned int *)nullptr, (int32_t *)nullptr);
    if ((s = scan_u32(M, (const unsigned int *)cnt, foff, nodes, st)) != RSM_OK) return s;
    if (trim) {
        dilate(d_occ, t0, 0);
        dilate((const uint8_t *)t0, t1, 1);
        dilate((const uint8_t *)t1, t0, 2);
    }
    uint64_t nv = 0, nf = 0;
    if ((s = scan_total(vcnt, vpos, nodes, st, &nv)) != RSM_OK) return s;
    if ((s = scan_total(cnt, foff, nodes, st, &nf)) != RSM_OK) return s;
    DEVCHK(hipGetLastError());
    untrimmed[0] = (int64_t)nv;
    untrimmed[1] = (int64_t)nf;
    if (nv == 0 || nf == 0) return RSM_OK;
    if (nv > (uint64_t)INT32_MAX || nf > (uint64_t)INT32_MAX / 3) return RSM_E_NOMEM;
    PoissonMesh full;
    if ((s = mesh_result_alloc(full, nv, nf)) != RSM_OK) return s;
    uint8_t *vkeep = trim ? M.get<uint8_t>(nv) : nullptr;
    if (!M.ok) {
        poisson_mesh_free(&full);
        return RSM_E_NOMEM;
    }
    hipLaunchKernelGGL(k_pv_emit_vertices<Space>, blocks_for(nodes), dim3(256), 0, st, d_chi, iso32, g, S, (const unsigned long long *)flag8, (const unsigned int *)vpos,
                       full.d_v, (const uint8_t *)t0, vkeep);
    hipLaunchKernelGGL((k_pv_cell_faces<true, Space>), blocks_for(nodes), dim3(256), 0, st, d_chi, iso32, S, tab, (unsigned int *)nullptr, (const unsigned int *)foff,
                       (const unsigned long long *)flag8, (const unsigned int *)vpos, full.d_f);
    if (!trim) {
        if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
            poisson_mesh_free(&full);
            return RSM_E_HIP;
        }
        *out = full;
        return RSM_OK;
    }
    return poisson_trim_commit(M, full, vkeep, out, st);
}
