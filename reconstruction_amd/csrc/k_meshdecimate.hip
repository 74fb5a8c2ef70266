// k_meshdecimate.hip -- decimation.mlx's "Quadric Edge Collapse Decimation" on the final mesh.  Not a bit-parity port of
// MeshLab / VCG (no source in the reference tree, and a serial priority queue is not what a GPU runs): every rule is defined in DESIGN.md 9
// (f13) and restated in numpy in tests/meshdecimate_restatement.py, and the kernels are held to that restatement exactly -- the same faces in
// the same order, the same float32 positions, the same fp64 quadrics and costs.
//   quadrics     once: per vertex the sum over its corner list, ascending, of the face's plane quadric and of the border planes of the two
//                edges of that corner                                                                   k_md_entry_border, k_md_quadrics
//   a round      mesh_common.h's sorted edge table -> the unique edges with their multiplicity, border and locked vertices     k_md_heads, k_md_unique, k_md_vertex
//                a thread per unique edge: link condition, duplicate faces, placement, error, quality, normals     k_md_costs
//                rank = the position in a stable sort by (cost bits, key order); the budget's participants;
//                m1 / m2 by integer atomicMin; the independent set                                                   k_md_rank, k_md_m2, k_md_select
//                the scan of the selected multiplicities cuts at `need`; b -> a, V[a] = x, Q[a] += Q[b]             k_md_apply
//                the faces through the map, those with a repeated index compacted away in order                     k_md_remap, k_md_compact
//   the end      the referenced vertices renumbered in ascending index                                              k_md_used, k_md_renumber
// fp64 + - * / sqrt only, no float atomics; built with -ffp-contract=off (csrc/Makefile): every expression is evaluated as written.  The ten
// quadric entries and the 3 x 3 solve live in named scalars: no kernel here uses scratch (profiles/f22_meshdecimate_resources.txt).
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"
#include "wave_prims.h"

#include <string.h>

#include <math.h>

#include <algorithm>

namespace {

typedef unsigned long long u64;

// reject codes (tests/meshdecimate_restatement.py has the same list); the placement branch goes into bits 4-5
enum { R_OK = 0, R_NONMANIFOLD, R_LOCKED, R_LINK, R_BORDER, R_DUPLICATE, R_NORMAL, R_NOTFINITE, R_N };
enum { B_OPTIMAL = 0, B_PA, B_PB, B_MID };
// counters: [1 .. 7] the rejects of a round by code; the rest as named.  C_VALENCE and C_MAXCOST run over the whole call.
enum { C_LOCKED = R_N, C_KEPT, C_BKEPT, C_SELECTED, C_VALENCE, C_MAXCOST, C_N };

#define MD_INF_BITS 0x7ff0000000000000ull
#define MD_K_QUALITY 3.4641016151377544 /* 2 sqrt(3) */

__device__ __forceinline__ bool finite64(double x) { return ((u64)__double_as_longlong(x) & MD_INF_BITS) != MD_INF_BITS; }
__device__ __forceinline__ bool finite32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ D3 sub3(const D3 &a, const D3 &b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(const D3 &a, const D3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross3(const D3 &u, const D3 &w) { return D3{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x}; }
__device__ __forceinline__ D3 sel3(int j, const D3 &a, const D3 &b, const D3 &c) { return j == 0 ? a : j == 1 ? b : c; }

// xx xy xz xd yy yz yd zz zd dd
struct Q10 {
    double q0, q1, q2, q3, q4, q5, q6, q7, q8, q9;
};
__device__ __forceinline__ void q_add_plane(Q10 &a, const D3 &n, double d) {
    a.q0 = a.q0 + n.x * n.x;
    a.q1 = a.q1 + n.x * n.y;
    a.q2 = a.q2 + n.x * n.z;
    a.q3 = a.q3 + n.x * d;
    a.q4 = a.q4 + n.y * n.y;
    a.q5 = a.q5 + n.y * n.z;
    a.q6 = a.q6 + n.y * d;
    a.q7 = a.q7 + n.z * n.z;
    a.q8 = a.q8 + n.z * d;
    a.q9 = a.q9 + d * d;
}
// the plane through the directed edge (pa, pb) perpendicular to the face with normal n, weighted; nothing for an edge without length
__device__ __forceinline__ void q_add_border(Q10 &a, const D3 &n, const D3 &pa, const D3 &pb, double bw) {
    const D3 e = sub3(pb, pa);
    const double L = sqrt(dot3(e, e));
    if (L == 0.0) return;
    const D3 c = cross3(n, e);
    const D3 m = D3{(bw * c.x) / L, (bw * c.y) / L, (bw * c.z) / L};
    q_add_plane(a, m, -dot3(m, pa));
}
__device__ __forceinline__ Q10 q_load(const double *__restrict__ Q, size_t v) {
    const double *q = Q + 10 * v;
    return Q10{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9]};
}
__device__ __forceinline__ void q_store(double *__restrict__ Q, size_t v, const Q10 &a) {
    double *q = Q + 10 * v;
    q[0] = a.q0; q[1] = a.q1; q[2] = a.q2; q[3] = a.q3; q[4] = a.q4;
    q[5] = a.q5; q[6] = a.q6; q[7] = a.q7; q[8] = a.q8; q[9] = a.q9;
}
__device__ __forceinline__ Q10 q_sum(const Q10 &a, const Q10 &b) {
    return Q10{a.q0 + b.q0, a.q1 + b.q1, a.q2 + b.q2, a.q3 + b.q3, a.q4 + b.q4, a.q5 + b.q5, a.q6 + b.q6, a.q7 + b.q7, a.q8 + b.q8, a.q9 + b.q9};
}
// (x, 1)^T Q (x, 1)
__device__ __forceinline__ double q_err(const Q10 &q, const D3 &p) {
    const double r0 = ((q.q0 * p.x + q.q1 * p.y) + q.q2 * p.z) + q.q3;
    const double r1 = ((q.q1 * p.x + q.q4 * p.y) + q.q5 * p.z) + q.q6;
    const double r2 = ((q.q2 * p.x + q.q5 * p.y) + q.q7 * p.z) + q.q8;
    const double r3 = ((q.q3 * p.x + q.q6 * p.y) + q.q8 * p.z) + q.q9;
    return ((p.x * r0 + p.y * r1) + p.z * r2) + r3;
}

// ---- tables ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_md_distinct(const int32_t *__restrict__ f, size_t nf, unsigned int *__restrict__ fkeep) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nf) fkeep[i] = face_distinct(f[3 * i], f[3 * i + 1], f[3 * i + 2]) ? 1u : 0u;
}
// the kept faces in order, their indices as they are
__global__ __launch_bounds__(256) void k_md_compact(const int32_t *__restrict__ f, size_t nf, const unsigned int *__restrict__ fkeep, const unsigned int *__restrict__ fpos,
                                                    int32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nf || !fkeep[i]) return;
    const size_t o = fpos[i];
    for (int c = 0; c < 3; c++) out[3 * o + c] = f[3 * i + c];
}

// per sorted position of the edge table: the entry of a run of length 1 is a border entry
__global__ __launch_bounds__(256) void k_md_entry_border(const u64 *__restrict__ key, const uint32_t *__restrict__ val, size_t n, u64 nv, uint8_t *__restrict__ isb) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    if ((k >> 32) == nv) return;
    if ((i > 0 && key[i - 1] == k) || (i + 1 < n && key[i + 1] == k)) return;
    isb[val[i]] = 1;
}

// Q_v: from 0 over v's corner list, ascending; per corner the face, then edge j, then edge (j + 2) % 3 where they are border edges
__global__ __launch_bounds__(256) void k_md_quadrics(const float *__restrict__ v, size_t nv, const int32_t *__restrict__ f, const uint32_t *__restrict__ row,
                                                     const uint32_t *__restrict__ corner, const uint8_t *__restrict__ isb, double bw, double *__restrict__ Q) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    Q10 acc = Q10{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t r = row[i]; r < row[i + 1]; r++) {
        const uint32_t c = corner[r];
        const size_t fi = c / 3;
        const int j = (int)(c % 3);
        const D3 p0 = ld3(v, (size_t)f[3 * fi]), p1 = ld3(v, (size_t)f[3 * fi + 1]), p2 = ld3(v, (size_t)f[3 * fi + 2]);
        const D3 n = cross3(sub3(p1, p0), sub3(p2, p0));
        q_add_plane(acc, n, -dot3(n, p0));
        const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        const D3 pj = sel3(j, p0, p1, p2);
        if (isb[3 * fi + j]) q_add_border(acc, n, pj, sel3(j1, p0, p1, p2), bw);
        if (isb[3 * fi + j2]) q_add_border(acc, n, sel3(j2, p0, p1, p2), pj, bw);
    }
    q_store(Q, i, acc);
}

// the first position of every run of the sorted edge table (the runs of the repeated-index key excluded)
__global__ __launch_bounds__(256) void k_md_heads(const u64 *__restrict__ key, size_t n, u64 nv, unsigned int *__restrict__ head) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    head[i] = ((k >> 32) != nv && (i == 0 || key[i - 1] != k)) ? 1u : 0u;
}
// the unique edges in key order with their multiplicity; the border and the locked vertices (stores of 1 only: any order gives the same)
__global__ __launch_bounds__(256) void k_md_unique(const u64 *__restrict__ key, size_t n, const unsigned int *__restrict__ head, const unsigned int *__restrict__ upos,
                                                   u64 *__restrict__ ukey, int32_t *__restrict__ mult, uint8_t *__restrict__ vborder, uint8_t *__restrict__ locked) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !head[i]) return;
    const u64 k = key[i];
    int m = 1;
    while (i + m < n && key[i + m] == k) m++;
    const size_t e = upos[i];
    ukey[e] = k;
    mult[e] = m;
    const size_t a = (size_t)(k >> 32), b = (size_t)(k & 0xffffffffull);
    if (m == 1) vborder[a] = vborder[b] = 1;
    if (m > 2) locked[a] = locked[b] = 1;
}

// a running maximum that many threads feed: the value only grows, so a thread that reads one at least as large as its own has nothing to add
__device__ __forceinline__ void ctr_max(u64 *p, u64 x) {
    if (x > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, x);
}
// preserve_boundary's locks; the locked vertices counted, the largest valence met (one atomic a wave each)
__global__ __launch_bounds__(256) void k_md_vertex(size_t nv, const uint32_t *__restrict__ row, const uint8_t *__restrict__ vborder, uint8_t *__restrict__ locked,
                                                   int preserve_boundary, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    u64 l = 0, val = 0;
    if (i < nv) {
        if (preserve_boundary && vborder[i]) locked[i] = 1;
        l = locked[i] ? 1 : 0;
        val = (u64)(row[i + 1] - row[i]);
    }
    l = wave_sum(l);
    val = wave_reduce(val, [](u64 x, u64 y) { return y > x ? y : x; });
    if ((threadIdx.x & 63) == 0) {
        if (l) atomicAdd(ctr + C_LOCKED, l);
        ctr_max(ctr + C_VALENCE, val);
    }
}

// ---- the cost of every unique edge ------------------------------------------------------------------------------------------------------------
struct CostParams {
    double quality_thr, min_error;
    int preserve_normal, preserve_topology, optimal_placement;
};

__device__ __forceinline__ bool face_has(const int32_t *__restrict__ f, size_t fi, int w) { return f[3 * fi] == w || f[3 * fi + 1] == w || f[3 * fi + 2] == w; }

// the position of the collapse: every candidate position is rounded to float32 first and judged as that
__device__ __forceinline__ int place(const Q10 &q, const D3 &pa, const D3 &pb, int optimal, float *xo, float *yo, float *zo) {
    const D3 mid = D3{(pa.x + pb.x) * 0.5, (pa.y + pb.y) * 0.5, (pa.z + pb.z) * 0.5};
    if (optimal) {
        // cofactors of the symmetric A = [q0 q1 q2; q1 q4 q5; q2 q5 q7], expanded along its first row; x = -(C b) / det, b = (q3, q6, q8)
        const double c00 = q.q4 * q.q7 - q.q5 * q.q5;
        const double c01 = q.q2 * q.q5 - q.q1 * q.q7;
        const double c02 = q.q1 * q.q5 - q.q4 * q.q2;
        const double c11 = q.q0 * q.q7 - q.q2 * q.q2;
        const double c12 = q.q1 * q.q2 - q.q0 * q.q5;
        const double c22 = q.q0 * q.q4 - q.q1 * q.q1;
        const double det = (q.q0 * c00 + q.q1 * c01) + q.q2 * c02;
        if (finite64(det) && det != 0.0) {
            const float fx = (float)(-(((c00 * q.q3 + c01 * q.q6) + c02 * q.q8) / det));
            const float fy = (float)(-(((c01 * q.q3 + c11 * q.q6) + c12 * q.q8) / det));
            const float fz = (float)(-(((c02 * q.q3 + c12 * q.q6) + c22 * q.q8) / det));
            if (finite32(fx) && finite32(fy) && finite32(fz)) {
                const D3 d = sub3(D3{(double)fx, (double)fy, (double)fz}, mid);
                const D3 e = sub3(pb, pa);
                if (dot3(d, d) <= 4.0 * dot3(e, e)) {
                    *xo = fx; *yo = fy; *zo = fz;
                    return B_OPTIMAL;
                }
            }
        }
    }
    const float mx = (float)mid.x, my = (float)mid.y, mz = (float)mid.z;
    const double ea = q_err(q, pa), eb = q_err(q, pb), em = q_err(q, D3{(double)mx, (double)my, (double)mz});
    int branch = B_PA;
    double best = ea;
    *xo = (float)pa.x; *yo = (float)pa.y; *zo = (float)pa.z;
    if (eb < best) {
        branch = B_PB;
        best = eb;
        *xo = (float)pb.x; *yo = (float)pb.y; *zo = (float)pb.z;
    }
    if (em < best) {
        branch = B_MID;
        *xo = mx; *yo = my; *zo = mz;
    }
    return branch;
}

// the faces at `at` without `other`, with `at` moved to x: the least quality and whether a normal turns over
__device__ __forceinline__ void star_walk(const float *__restrict__ v, const int32_t *__restrict__ f, const uint32_t *__restrict__ row, const uint32_t *__restrict__ corner,
                                          int at, int other, const D3 &x, double &minq, bool &flipped) {
    for (uint32_t r = row[at]; r < row[at + 1]; r++) {
        const size_t fi = corner[r] / 3;
        if (face_has(f, fi, other)) continue;
        const int i0 = f[3 * fi], i1 = f[3 * fi + 1], i2 = f[3 * fi + 2];
        const D3 o0 = ld3(v, (size_t)i0), o1 = ld3(v, (size_t)i1), o2 = ld3(v, (size_t)i2);
        const D3 n0 = i0 == at ? x : o0, n1 = i1 == at ? x : o1, n2 = i2 == at ? x : o2;
        const D3 nold = cross3(sub3(o1, o0), sub3(o2, o0));
        const D3 nnew = cross3(sub3(n1, n0), sub3(n2, n0));
        if (!(dot3(nnew, nold) > 0.0)) flipped = true;
        const double nn = dot3(nnew, nnew);
        const D3 e0 = sub3(n1, n0), e1 = sub3(n2, n1), e2 = sub3(n0, n2);
        const double s = (dot3(e0, e0) + dot3(e1, e1)) + dot3(e2, e2);
        const double q = (nn > 0.0 && s > 0.0) ? (MD_K_QUALITY * sqrt(nn)) / s : 0.0;
        minq = q < minq ? q : minq;
    }
}

__global__ __launch_bounds__(256) void k_md_costs(const float *__restrict__ v, const int32_t *__restrict__ f, const double *__restrict__ Q, const uint32_t *__restrict__ row,
                                                  const uint32_t *__restrict__ corner, const u64 *__restrict__ ukey, const int32_t *__restrict__ mult, size_t ne,
                                                  const uint8_t *__restrict__ vborder, const uint8_t *__restrict__ locked, CostParams P, u64 *__restrict__ cbits,
                                                  uint32_t *__restrict__ eidx, int32_t *__restrict__ reject, float *__restrict__ pos, u64 *__restrict__ ctr) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const u64 k = ukey[e];
    const int a = (int)(k >> 32), b = (int)(k & 0xffffffffull);
    const int m = mult[e];
    const uint32_t ra0 = row[a], ra1 = row[a + 1], rb0 = row[b], rb1 = row[b + 1];
    int code = R_OK;
    if (m > 2) code = R_NONMANIFOLD;
    else if (locked[a] | locked[b]) code = R_LOCKED;
    if (code == R_OK && P.preserve_topology) {
        // the distinct neighbours of a that are neighbours of b as well
        int common = 0;
        for (uint32_t r = ra0; r < ra1; r++) {
            const uint32_t c = corner[r];
            const size_t fi = c / 3;
            const int j = (int)(c % 3);
            for (int t = 1; t <= 2; t++) {
                const int w = f[3 * fi + (j + t) % 3];
                if (w == b) continue;
                bool seen = false; // in an earlier face of a's list
                for (uint32_t r2 = ra0; r2 < r && !seen; r2++) seen = face_has(f, corner[r2] / 3, w);
                if (seen) continue;
                bool atb = false;
                for (uint32_t r3 = rb0; r3 < rb1 && !atb; r3++) atb = face_has(f, corner[r3] / 3, w);
                common += atb ? 1 : 0;
            }
        }
        if (common != m) code = R_LINK;
        else if (vborder[a] && vborder[b] && m != 1) code = R_BORDER;
    }
    if (code == R_OK) {
        // two surviving faces with the same three vertices: (a, c, d) and (b, c, d) both exist
        bool dup = false;
        for (uint32_t r = ra0; r < ra1 && !dup; r++) {
            const uint32_t c = corner[r];
            const size_t fi = c / 3;
            const int j = (int)(c % 3);
            const int c1 = f[3 * fi + (j + 1) % 3], d1 = f[3 * fi + (j + 2) % 3];
            if (c1 == b || d1 == b) continue;
            for (uint32_t r3 = rb0; r3 < rb1 && !dup; r3++) {
                const uint32_t cc = corner[r3];
                const size_t f3 = cc / 3;
                const int j3 = (int)(cc % 3);
                const int c2 = f[3 * f3 + (j3 + 1) % 3], d2 = f[3 * f3 + (j3 + 2) % 3];
                dup = (c1 == c2 && d1 == d2) || (c1 == d2 && d1 == c2);
            }
        }
        if (dup) code = R_DUPLICATE;
    }
    double cost = __longlong_as_double((long long)MD_INF_BITS);
    float fx = 0.0f, fy = 0.0f, fz = 0.0f;
    int branch = 0;
    if (code == R_OK) {
        const Q10 q = q_sum(q_load(Q, (size_t)a), q_load(Q, (size_t)b));
        const D3 pa = ld3(v, (size_t)a), pb = ld3(v, (size_t)b);
        branch = place(q, pa, pb, P.optimal_placement, &fx, &fy, &fz);
        const D3 x = D3{(double)fx, (double)fy, (double)fz};
        double err = q_err(q, x);
        double minq = 1.0;
        bool flipped = false;
        star_walk(v, f, row, corner, a, b, x, minq, flipped);
        star_walk(v, f, row, corner, b, a, x, minq, flipped);
        if (P.preserve_normal && flipped) code = R_NORMAL;
        else if (!finite64(err)) code = R_NOTFINITE;
        else {
            err = err > P.min_error ? err : P.min_error;
            double c = err;
            if (P.quality_thr > 0.0) {
                double cl = minq < 1e-8 ? 1e-8 : minq;
                cl = cl > P.quality_thr ? P.quality_thr : cl;
                c = err / cl;
            }
            if (!finite64(c)) code = R_NOTFINITE;
            else cost = c;
        }
        code |= branch << 4;
    }
    cbits[e] = (u64)__double_as_longlong(cost);
    eidx[e] = (uint32_t)e;
    reject[e] = code;
    pos[3 * e] = fx;
    pos[3 * e + 1] = fy;
    pos[3 * e + 2] = fz;
    if (code & 15) atomicAdd(ctr + (code & 15), (u64)1);
}

// ---- selection --------------------------------------------------------------------------------------------------------------------------------
// per rank r: the edge at r; a participant (a candidate of rank below the budget) lowers m1 of its endpoints to r
__global__ __launch_bounds__(256) void k_md_rank(const u64 *__restrict__ sbits, const uint32_t *__restrict__ ord, size_t ne, u64 budget, const u64 *__restrict__ ukey,
                                                 unsigned int *__restrict__ m1) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= ne || (u64)r >= budget || sbits[r] >= MD_INF_BITS) return;
    const u64 k = ukey[ord[r]];
    atomicMin(m1 + (size_t)(k >> 32), (unsigned int)r);
    atomicMin(m1 + (size_t)(k & 0xffffffffull), (unsigned int)r);
}
// m2 (which starts as a copy of m1): the least m1 over a vertex and its neighbours
__global__ __launch_bounds__(256) void k_md_m2(const u64 *__restrict__ ukey, size_t ne, const unsigned int *__restrict__ m1, unsigned int *__restrict__ m2) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const u64 k = ukey[e];
    const size_t a = (size_t)(k >> 32), b = (size_t)(k & 0xffffffffull);
    const unsigned int ma = m1[a], mb = m1[b];
    if (mb != 0xffffffffu) atomicMin(m2 + a, mb);
    if (ma != 0xffffffffu) atomicMin(m2 + b, ma);
}
// per rank r: selected iff a participant with r = m2(a) = m2(b); selm = its multiplicity (0: not selected)
__global__ __launch_bounds__(256) void k_md_select(const u64 *__restrict__ sbits, const uint32_t *__restrict__ ord, size_t ne, u64 budget, const u64 *__restrict__ ukey,
                                                   const int32_t *__restrict__ mult, const unsigned int *__restrict__ m2, unsigned int *__restrict__ selm,
                                                   unsigned int *__restrict__ self) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= ne) return;
    unsigned int s = 0u;
    if ((u64)r < budget && sbits[r] < MD_INF_BITS) {
        const uint32_t e = ord[r];
        const u64 k = ukey[e];
        if (m2[(size_t)(k >> 32)] == (unsigned int)r && m2[(size_t)(k & 0xffffffffull)] == (unsigned int)r) s = (unsigned int)mult[e];
    }
    selm[r] = s;
    self[r] = s ? 1u : 0u;
}
// per rank r: a selected edge is kept while the faces the edges before it remove are fewer than need: b -> a, V[a] = x, Q[a] += Q[b].
// Selected edges share no endpoint, so every vertex written here has one writer.  sel (may be NULL): the selected keys in rank order.
__global__ __launch_bounds__(256) void k_md_apply(const u64 *__restrict__ sbits, const uint32_t *__restrict__ ord, size_t ne, const u64 *__restrict__ ukey,
                                                  const unsigned int *__restrict__ selm, const unsigned int *__restrict__ sscan, const unsigned int *__restrict__ spos,
                                                  u64 need, const float *__restrict__ pos, float *__restrict__ v, double *__restrict__ Q, int *__restrict__ vmap,
                                                  u64 *__restrict__ sel, u64 *__restrict__ ctr) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= ne || !selm[r]) return;
    const uint32_t e = ord[r];
    const u64 k = ukey[e];
    if (sel) sel[spos[r]] = k;
    atomicAdd(ctr + C_SELECTED, (u64)1);
    if ((u64)sscan[r] >= need) return;
    const size_t a = (size_t)(k >> 32), b = (size_t)(k & 0xffffffffull);
    vmap[b] = (int)a;
    for (int c = 0; c < 3; c++) v[3 * a + c] = pos[3 * (size_t)e + c];
    q_store(Q, a, q_sum(q_load(Q, a), q_load(Q, b)));
    atomicAdd(ctr + C_KEPT, (u64)1);
    if (selm[r] == 1u) atomicAdd(ctr + C_BKEPT, (u64)1);
    ctr_max(ctr + C_MAXCOST, sbits[r]); // (costs are not negative: their bits order as they do)
}
__global__ __launch_bounds__(256) void k_md_remap(const int32_t *__restrict__ f, size_t nf, const int *__restrict__ vmap, int32_t *__restrict__ g,
                                                  unsigned int *__restrict__ fkeep) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const int a = vmap[f[3 * i]], b = vmap[f[3 * i + 1]], c = vmap[f[3 * i + 2]];
    g[3 * i] = a;
    g[3 * i + 1] = b;
    g[3 * i + 2] = c;
    fkeep[i] = face_distinct(a, b, c) ? 1u : 0u;
}

// ---- the end: the referenced vertices, renumbered ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_md_used(const int32_t *__restrict__ f, size_t n, unsigned int *__restrict__ vused) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) vused[f[i]] = 1u;
}
__global__ __launch_bounds__(256) void k_md_renumber(const int32_t *__restrict__ f, size_t n, const unsigned int *__restrict__ vpos, int32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int32_t)vpos[f[i]];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
// the tables of a mesh and the cost of its unique edges
struct Round {
    size_t ne = 0;
    u64 *ekey = nullptr, *ukey = nullptr, *cbits = nullptr;
    uint32_t *eval = nullptr, *row = nullptr, *corner = nullptr, *eidx = nullptr;
    int32_t *mult = nullptr, *reject = nullptr;
    uint8_t *vborder = nullptr, *locked = nullptr;
    float *pos = nullptr;
};

// both of mesh_common.h's tables
template <class Alloc>
static int tables(Alloc &M, Round &T, const int32_t *d_f, size_t nv, size_t nf, hipStream_t st) {
    const size_t n = 3 * nf;
    u64 *k0 = M.template get<u64>(n);
    uint32_t *v0 = M.template get<uint32_t>(n);
    T.ekey = M.template get<u64>(n);
    T.eval = M.template get<uint32_t>(n);
    if (!k0 || !v0 || !T.ekey || !T.eval) return RSM_E_NOMEM;
    const int s = mesh_edge_table(M, d_f, nv, nf, k0, v0, T.ekey, T.eval, st);
    return s != RSM_OK ? s : mesh_corner_lists(M, d_f, nv, nf, &T.row, &T.corner, st);
}

// nv > 0, nf > 0, a validated mesh
template <class Alloc>
static int quadrics(Alloc &M, const float *d_v, size_t nv, const int32_t *d_f, size_t nf, double bw, double *d_q, hipStream_t st) {
    Round T;
    int s = tables(M, T, d_f, nv, nf, st);
    if (s != RSM_OK) return s;
    uint8_t *isb = M.template get<uint8_t>(3 * nf);
    if (!isb) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(isb, 0, 3 * nf, st));
    hipLaunchKernelGGL(k_md_entry_border, blocks_for(3 * nf), dim3(256), 0, st, (const u64 *)T.ekey, (const uint32_t *)T.eval, 3 * nf, (u64)nv, isb);
    hipLaunchKernelGGL(k_md_quadrics, blocks_for(nv), dim3(256), 0, st, d_v, nv, d_f, (const uint32_t *)T.row, (const uint32_t *)T.corner, (const uint8_t *)isb, bw, d_q);
    return RSM_OK;
}

// the unique edges of the mesh and their costs; ctr: C_N counters, the per-round ones zeroed here.  One host round trip (the edge count).
template <class Alloc>
static int costs(Alloc &M, Round &T, const float *d_v, size_t nv, const int32_t *d_f, size_t nf, const double *d_q, const rsm_mesh_decimate_params *p, u64 *ctr,
                 hipStream_t st) {
    const size_t n = 3 * nf;
    int s = tables(M, T, d_f, nv, nf, st);
    if (s != RSM_OK) return s;
    unsigned int *head = M.template get<unsigned int>(n), *upos = M.template get<unsigned int>(n);
    T.vborder = M.template get<uint8_t>(nv);
    T.locked = M.template get<uint8_t>(nv);
    if (!head || !upos || !T.vborder || !T.locked) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(ctr, 0, C_VALENCE * sizeof(u64), st));
    DEVCHK(hipMemsetAsync(T.vborder, 0, nv, st));
    DEVCHK(hipMemsetAsync(T.locked, 0, nv, st));
    hipLaunchKernelGGL(k_md_heads, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, n, (u64)nv, head);
    if ((s = scan_u32(M, (const unsigned int *)head, upos, n, st)) != RSM_OK) return s;
    uint64_t ne = 0;
    if ((s = scan_total(head, upos, n, st, &ne)) != RSM_OK) return s;
    T.ne = (size_t)ne;
    T.ukey = M.template get<u64>(ne);
    T.mult = M.template get<int32_t>(ne);
    T.cbits = M.template get<u64>(ne);
    T.eidx = M.template get<uint32_t>(ne);
    T.reject = M.template get<int32_t>(ne);
    T.pos = M.template get<float>(3 * ne);
    if (!T.ukey || !T.mult || !T.cbits || !T.eidx || !T.reject || !T.pos) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_md_unique, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, n, (const unsigned int *)head, (const unsigned int *)upos, T.ukey, T.mult,
                       T.vborder, T.locked);
    hipLaunchKernelGGL(k_md_vertex, blocks_for(nv), dim3(256), 0, st, nv, (const uint32_t *)T.row, (const uint8_t *)T.vborder, T.locked, p->preserve_boundary, ctr);
    if (ne > 0) {
        const CostParams P = {p->quality_thr, p->min_error, p->preserve_normal, p->preserve_topology, p->optimal_placement};
        hipLaunchKernelGGL(k_md_costs, blocks_for(ne), dim3(256), 0, st, d_v, d_f, d_q, (const uint32_t *)T.row, (const uint32_t *)T.corner, (const u64 *)T.ukey,
                           (const int32_t *)T.mult, (size_t)ne, (const uint8_t *)T.vborder, (const uint8_t *)T.locked, P, T.cbits, T.eidx, T.reject, T.pos, ctr);
    }
    return RSM_OK;
}

// One round on a mesh without repeated-index faces... or with: they take no part and go with the compaction.  d_v and d_q are updated in
// place, the faces go from d_f to d_fout (room for nf) through d_ftmp (room for nf); h: the counters after the round; d_sel (may be NULL):
// room for the selected keys.  need > 0, nv > 0, nf > 0.
template <class Alloc>
static int round_run(Alloc &M, float *d_v, size_t nv, double *d_q, const int32_t *d_f, size_t nf, int32_t *d_ftmp, int32_t *d_fout, u64 need,
                     const rsm_mesh_decimate_params *p, u64 *ctr, u64 *h, size_t *nf_out, u64 *d_sel, hipStream_t st) {
    Round T;
    int s = costs(M, T, d_v, nv, d_f, nf, d_q, p, ctr, st);
    if (s != RSM_OK) return s;
    const size_t ne = T.ne;
    unsigned int *fkeep = M.template get<unsigned int>(nf), *fpos = M.template get<unsigned int>(nf);
    int *vmap = M.template get<int>(nv);
    if (!fkeep || !fpos || !vmap) return RSM_E_NOMEM;
    hipLaunchKernelGGL(k_mesh_iota<>, blocks_for(nv), dim3(256), 0, st, vmap, nv);
    if (ne > 0) {
        u64 *sbits = M.template get<u64>(ne);
        uint32_t *ord = M.template get<uint32_t>(ne);
        unsigned int *m1 = M.template get<unsigned int>(nv), *m2 = M.template get<unsigned int>(nv);
        unsigned int *selm = M.template get<unsigned int>(ne), *self = M.template get<unsigned int>(ne), *sscan = M.template get<unsigned int>(ne),
                     *spos = M.template get<unsigned int>(ne);
        if (!sbits || !ord || !m1 || !m2 || !selm || !self || !sscan || !spos) return RSM_E_NOMEM;
        if ((s = sort_pairs(M, T.cbits, sbits, T.eidx, ord, ne, 64, st)) != RSM_OK) return s;
        const u64 budget = (need + 1) / 2;
        DEVCHK(hipMemsetAsync(m1, 0xff, nv * sizeof(unsigned int), st));
        hipLaunchKernelGGL(k_md_rank, blocks_for(ne), dim3(256), 0, st, (const u64 *)sbits, (const uint32_t *)ord, ne, budget, (const u64 *)T.ukey, m1);
        DEVCHK(hipMemcpyAsync(m2, m1, nv * sizeof(unsigned int), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_md_m2, blocks_for(ne), dim3(256), 0, st, (const u64 *)T.ukey, ne, (const unsigned int *)m1, m2);
        hipLaunchKernelGGL(k_md_select, blocks_for(ne), dim3(256), 0, st, (const u64 *)sbits, (const uint32_t *)ord, ne, budget, (const u64 *)T.ukey,
                           (const int32_t *)T.mult, (const unsigned int *)m2, selm, self);
        if ((s = scan_u32(M, (const unsigned int *)selm, sscan, ne, st)) != RSM_OK || (s = scan_u32(M, (const unsigned int *)self, spos, ne, st)) != RSM_OK) return s;
        hipLaunchKernelGGL(k_md_apply, blocks_for(ne), dim3(256), 0, st, (const u64 *)sbits, (const uint32_t *)ord, ne, (const u64 *)T.ukey, (const unsigned int *)selm,
                           (const unsigned int *)sscan, (const unsigned int *)spos, need, (const float *)T.pos, d_v, d_q, vmap, d_sel, ctr);
    }
    hipLaunchKernelGGL(k_md_remap, blocks_for(nf), dim3(256), 0, st, d_f, nf, (const int *)vmap, d_ftmp, fkeep);
    if ((s = scan_u32(M, (const unsigned int *)fkeep, fpos, nf, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_md_compact, blocks_for(nf), dim3(256), 0, st, (const int32_t *)d_ftmp, nf, (const unsigned int *)fkeep, (const unsigned int *)fpos, d_fout);
    DEVCHK(hipMemcpyAsync(h, ctr, C_N * sizeof(u64), hipMemcpyDeviceToHost, st));
    uint64_t kept = 0;
    if ((s = scan_total(fkeep, fpos, nf, st, &kept)) != RSM_OK) return s; // (the round's one other round trip; the counters came with it)
    *nf_out = (size_t)kept;
    return RSM_OK;
}

static size_t pool_block(size_t nv, size_t nf) { return 160 * 3 * nf + 32 * nv + ((size_t)1 << 20); }

} // namespace

int mesh_quadrics_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, double boundary_weight, double *d_q, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK || nv == 0) return s;
    DEVCHK(hipMemsetAsync(d_q, 0, 10 * nv * sizeof(double), st));
    DevMem M;
    if (nf > 0 && (s = quadrics(M, d_v, nv, d_f, nf, boundary_weight, d_q, st)) != RSM_OK) return s;
    return mesh_finish(st);
}

int mesh_collapse_costs_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const double *d_q, const rsm_mesh_decimate_params *p, uint64_t *d_key,
                               int32_t *d_mult, double *d_cost, int32_t *d_reject, float *d_pos, int64_t *n_edges, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    *n_edges = 0;
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK || nv == 0 || nf == 0) return s;
    DevMem M;
    Round T;
    u64 *ctr = M.get<u64>(C_N);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(ctr, 0, C_N * sizeof(u64), st));
    if ((s = costs(M, T, d_v, nv, d_f, nf, d_q, p, ctr, st)) != RSM_OK) return s;
    if (T.ne > 0) {
        DEVCHK(hipMemcpyAsync(d_key, T.ukey, T.ne * sizeof(u64), hipMemcpyDeviceToDevice, st));
        DEVCHK(hipMemcpyAsync(d_mult, T.mult, T.ne * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        DEVCHK(hipMemcpyAsync(d_cost, T.cbits, T.ne * sizeof(u64), hipMemcpyDeviceToDevice, st));
        DEVCHK(hipMemcpyAsync(d_reject, T.reject, T.ne * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        DEVCHK(hipMemcpyAsync(d_pos, T.pos, 3 * T.ne * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    *n_edges = (int64_t)T.ne;
    return mesh_finish(st);
}

int mesh_collapse_round_device(float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, double *d_q, const rsm_mesh_decimate_params *p, int64_t need, int32_t *d_fout,
                               int64_t *nf_out, uint64_t *d_sel, int64_t *n_selected, int64_t *n_kept, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    *nf_out = *n_selected = *n_kept = 0;
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK || nv == 0 || nf == 0) return s;
    DevMem M;
    u64 *ctr = M.get<u64>(C_N);
    int32_t *ftmp = M.get<int32_t>(3 * nf);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(ctr, 0, C_N * sizeof(u64), st));
    u64 h[C_N] = {0};
    size_t kept_faces = 0;
    if (need > 0) {
        if ((s = round_run(M, d_v, nv, d_q, d_f, nf, ftmp, d_fout, (u64)need, p, ctr, h, &kept_faces, (u64 *)d_sel, st)) != RSM_OK) return s;
    } else { // nothing to remove: the faces without those of a repeated index
        unsigned int *fkeep = M.get<unsigned int>(nf), *fpos = M.get<unsigned int>(nf);
        if (!M.ok) return RSM_E_NOMEM;
        hipLaunchKernelGGL(k_md_distinct, blocks_for(nf), dim3(256), 0, st, d_f, nf, fkeep);
        if ((s = scan_u32(M, (const unsigned int *)fkeep, fpos, nf, st)) != RSM_OK) return s;
        hipLaunchKernelGGL(k_md_compact, blocks_for(nf), dim3(256), 0, st, d_f, nf, (const unsigned int *)fkeep, (const unsigned int *)fpos, d_fout);
        uint64_t k = 0;
        if ((s = scan_total(fkeep, fpos, nf, st, &k)) != RSM_OK) return s;
        kept_faces = (size_t)k;
    }
    *nf_out = (int64_t)kept_faces;
    *n_selected = (int64_t)h[C_SELECTED];
    *n_kept = (int64_t)h[C_KEPT];
    return mesh_finish(st);
}

int mesh_decimate_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const rsm_mesh_decimate_params *p, PoissonMesh *out, double *stats, int *invalid,
                         hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    double S[RSM_MESH_DECIMATE_STATS] = {0};
    S[0] = (double)nv;
    S[1] = (double)nf;
    const int64_t target = p->target_fraction > 0.0 ? (int64_t)floor(p->target_fraction * (double)nf_) : p->target_faces;
    S[19] = (double)target;
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK) return s;
    DevMem M;
    PoissonMesh res;
    u64 h[C_N] = {0};
    size_t cur_nf = 0;
    if (nv > 0 && nf > 0) {
        // the working mesh: positions, quadrics, two face buffers and the remap's
        float *V = M.get<float>(3 * nv);
        int32_t *F[2] = {M.get<int32_t>(3 * nf), M.get<int32_t>(3 * nf)}, *ftmp = M.get<int32_t>(3 * nf);
        unsigned int *fkeep = M.get<unsigned int>(nf), *fpos = M.get<unsigned int>(nf), *vused = M.get<unsigned int>(nv), *vpos = M.get<unsigned int>(nv);
        u64 *ctr = M.get<u64>(C_N);
        if (!M.ok) return RSM_E_NOMEM;
        DEVCHK(hipMemsetAsync(ctr, 0, C_N * sizeof(u64), st));
        DEVCHK(hipMemcpyAsync(V, d_v, 3 * nv * sizeof(float), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_md_distinct, blocks_for(nf), dim3(256), 0, st, d_f, nf, fkeep);
        if ((s = scan_u32(M, (const unsigned int *)fkeep, fpos, nf, st)) != RSM_OK) return s;
        hipLaunchKernelGGL(k_md_compact, blocks_for(nf), dim3(256), 0, st, d_f, nf, (const unsigned int *)fkeep, (const unsigned int *)fpos, F[0]);
        uint64_t k = 0;
        if ((s = scan_total(fkeep, fpos, nf, st, &k)) != RSM_OK) return s;
        cur_nf = (size_t)k;
        S[4] = (double)(nf - cur_nf);
        int cur = 0;
        if (cur_nf > 0 && (int64_t)cur_nf > target) {
            double *Q = M.get<double>(10 * nv);
            if (!M.ok) return RSM_E_NOMEM;
            Pool R(pool_block(nv, cur_nf));
            if ((s = quadrics(R, V, nv, F[0], cur_nf, p->boundary_weight, Q, st)) != RSM_OK) return s;
            int rounds = 0;
            double collapses = 0.0, border = 0.0;
            while ((int64_t)cur_nf > target && rounds < p->max_rounds) {
                R.rewind(); // (the stream is in order: the kernels of the round before are done with these pieces before the next ones write them)
                size_t next_nf = 0;
                if ((s = round_run(R, V, nv, Q, F[cur], cur_nf, ftmp, F[cur ^ 1], (u64)((int64_t)cur_nf - target), p, ctr, h, &next_nf, nullptr, st)) != RSM_OK) return s;
                rounds++;
                if (h[C_KEPT] == 0) break; // no candidate is left
                collapses += (double)h[C_KEPT];
                border += (double)h[C_BKEPT];
                cur ^= 1;
                cur_nf = next_nf;
            }
            S[5] = (double)rounds;
            S[6] = collapses;
            S[7] = border;
        }
        // AutoClean: the referenced vertices in ascending index
        uint64_t kv = 0;
        if (cur_nf > 0) {
            DEVCHK(hipMemsetAsync(vused, 0, nv * sizeof(unsigned int), st));
            hipLaunchKernelGGL(k_md_used, blocks_for(3 * cur_nf), dim3(256), 0, st, (const int32_t *)F[cur], 3 * cur_nf, vused);
            if ((s = scan_u32(M, (const unsigned int *)vused, vpos, nv, st)) != RSM_OK || (s = scan_total(vused, vpos, nv, st, &kv)) != RSM_OK) return s;
            if ((s = mesh_result_alloc(res, (size_t)kv, cur_nf)) != RSM_OK) return s;
            hipLaunchKernelGGL(k_md_renumber, blocks_for(3 * cur_nf), dim3(256), 0, st, (const int32_t *)F[cur], 3 * cur_nf, (const unsigned int *)vpos, res.d_f);
            hipLaunchKernelGGL(k_mesh_compact_verts<>, blocks_for(nv), dim3(256), 0, st, (const float *)V, nv, (const unsigned int *)vused, (const unsigned int *)vpos, res.d_v);
        }
        if (mesh_finish(st) != RSM_OK) {
            poisson_mesh_free(&res);
            return RSM_E_HIP;
        }
    }
    S[2] = (double)res.nv;
    S[3] = (double)res.nf;
    for (int c = 1; c < R_N; c++) S[7 + c] = (double)h[c];
    S[15] = (double)h[C_LOCKED];
    S[16] = (double)h[C_VALENCE];
    double maxcost;
    memcpy(&maxcost, &h[C_MAXCOST], sizeof maxcost);
    S[17] = maxcost;
    S[18] = res.nf <= target ? 1.0 : 0.0;
    if (stats) memcpy(stats, S, sizeof S);
    mesh_result_commit(out, res);
    return RSM_OK;
}
