// k_meshsubdivide.hip -- subdiv.mlx's "Subdivision Surfaces: Loop" on the final mesh.  Not a bit-parity port of MeshLab /
// VCG (no source in the reference tree): every rule is defined in DESIGN.md 9 (f15) and restated in numpy in
// tests/meshsubdivide_restatement.py, and the kernels are held to that restatement exactly -- the same faces in the same order, the same
// float32 positions.  Only Loop's own weights (MeshLab's LoopWeight 0) are built: LoopWeight 1 and 2 ("Enhance regularity", "Enhance
// continuity"; subdiv.mlx selects 2) rest on VCG's weight tables, which the reference tree does not hold; weight_scheme != 0 is refused.
//   an iteration  mesh_common.h's sorted edge table and corner lists
//                 a thread per sorted entry: the head of a run decides whether its edge splits (strictly longer than thr) and feeds the
//                 integer counts behind the vertex classes                                                                  k_sd_edges
//                 the rank of the split edges by a scan; the new vertex nv + rank written to every entry of the run         k_sd_marks
//                 a thread per vertex: locked / border / interior, whether it moves                                         k_sd_vertex
//                 a thread per face: 1 + its split edges faces; the scan of that                                            k_sd_count, k_sd_totals
//                 the one read-back: split edges, faces out, the counters
//                 a thread per split edge: the odd point; a thread per vertex: the even point                               k_sd_odd, k_sd_even
//                 a thread per face: its 1..4 faces in place, the quad of the two-split pattern cut by the output positions k_sd_emit
// fp64 + - * only (beta_k comes from the host's libm: BetaTable), float32 at the final store, no float atomics, no union-find, every loop
// bounded by a run or a corner list; built with -ffp-contract=off (csrc/Makefile): every expression is evaluated as written.  An iteration
// allocates its scratch -- one block (mesh_common.h's Pool) -- before its first launch and its result right behind the read-back, when the
// stream is empty.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "mesh_common.h"
#include "subdivide_limits.h"
#include "wave_prims.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

namespace {

typedef unsigned long long u64;

// vertex classes (tests/meshsubdivide_restatement.py has the same list); V_MOVES is set beside the class where the vertex moves
enum { V_INTERIOR = 0, V_BORDER = 1, V_LOCKED = 2, V_MOVES = 4 };
// per-vertex flags the edges set
enum { VF_MANY = 1, VF_SPLIT = 2 };
// the counters of one iteration
enum { C_NSPLIT, C_NFOUT, C_SPLIT_BORDER, C_SPLIT_MANY, C_PAT0, C_PAT1, C_PAT2, C_PAT3, C_MOVED_INTERIOR, C_MOVED_BORDER, C_LOCKED, C_VALENCE, C_N };

__device__ __forceinline__ D3 add3(const D3 &a, const D3 &b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 mul3(const D3 &a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dist2(const D3 &a, const D3 &b) {
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ void st3(float *__restrict__ v, size_t i, const D3 &p) {
    v[3 * i] = (float)p.x;
    v[3 * i + 1] = (float)p.y;
    v[3 * i + 2] = (float)p.z;
}
// the vertex opposite the edge of entry e = 3 f + j
__device__ __forceinline__ int opposite(const int32_t *__restrict__ f, uint32_t e) { return f[3 * (size_t)(e / 3) + (e % 3 + 2) % 3]; }

// ---- the edges: which split, and what the vertices learn from them -----------------------------------------------------------------------------
// per sorted position: sflag = 1 at the head of the run of an edge that splits.  A border edge (one face) counts at both ends and leaves
// the other end there as a minimum and in a sum (two border edges: the two neighbours); an edge of three or more faces and a split edge
// set their bit at both ends.  Integer atomics only: any order gives the same.
__global__ __launch_bounds__(256) void k_sd_edges(const u64 *__restrict__ key, size_t n, u64 nv, const float *__restrict__ v, double thr2, unsigned int *__restrict__ sflag,
                                                  unsigned int *__restrict__ nbord, unsigned int *__restrict__ vflag, unsigned int *__restrict__ bmin,
                                                  unsigned int *__restrict__ bsum, u64 *__restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    u64 k = 0;
    bool head = false;
    if (i < n) {
        k = key[i];
        head = (k >> 32) != nv && (i == 0 || key[i - 1] != k);
    }
    u64 s = 0, sb = 0, sm = 0;
    if (head) {
        int m = 1; // 1, 2, or 3 for three and more
        while (m < 3 && i + m < n && key[i + m] == k) m++;
        const unsigned int a = (unsigned int)(k >> 32), b = (unsigned int)(k & 0xffffffffull);
        if (dist2(ld3(v, a), ld3(v, b)) > thr2) s = 1;
        if (m == 1) {
            atomicAdd(nbord + a, 1u);
            atomicAdd(nbord + b, 1u);
            atomicMin(bmin + a, b);
            atomicMin(bmin + b, a);
            atomicAdd(bsum + a, b);
            atomicAdd(bsum + b, a);
        }
        const unsigned int fl = (m == 3 ? (unsigned int)VF_MANY : 0u) | (s ? (unsigned int)VF_SPLIT : 0u);
        if (fl) {
            atomicOr(vflag + a, fl);
            atomicOr(vflag + b, fl);
        }
        sb = (s && m == 1) ? 1 : 0;
        sm = (s && m == 3) ? 1 : 0;
    }
    if (i < n) sflag[i] = (unsigned int)s;
    const u64 packed = wave_sum(sb | (sm << 32)); // (at most 64 of each a wave)
    if ((threadIdx.x & 63) == 0 && packed) {
        if (packed & 0xffffffffull) atomicAdd(ctr + C_SPLIT_BORDER, packed & 0xffffffffull);
        if (packed >> 32) atomicAdd(ctr + C_SPLIT_MANY, packed >> 32);
    }
}

// the r-th split edge in key order: its head's position into slist[r], the new vertex nv + r into emid of every entry of its run
__global__ __launch_bounds__(256) void k_sd_marks(const u64 *__restrict__ key, const uint32_t *__restrict__ val, size_t n, u64 nv, const unsigned int *__restrict__ sflag,
                                                  const unsigned int *__restrict__ srank, uint32_t *__restrict__ slist, int32_t *__restrict__ emid) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !sflag[i]) return;
    const u64 k = key[i];
    const unsigned int r = srank[i];
    slist[r] = (uint32_t)i;
    const int32_t mid = (int32_t)(nv + r);
    for (size_t t = i; t < n && key[t] == k; t++) emid[val[t]] = mid;
}

__device__ __forceinline__ void ctr_max(u64 *p, u64 x) {
    if (x > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, x);
}

// the class of every vertex, and whether it moves: not locked and at an edge that splits.  A grid of at most COUNT_BLOCKS blocks strides over
// the vertices, so that the counters take a few thousand atomics whatever the size of the mesh (a wave an atomic cost 2 ms of a 10 ms call)
__global__ __launch_bounds__(256) void k_sd_vertex(size_t nv, const uint32_t *__restrict__ row, const unsigned int *__restrict__ nbord, const unsigned int *__restrict__ vflag,
                                                   uint8_t *__restrict__ vclass, u64 *__restrict__ ctr) {
    u64 mi = 0, mb = 0, lk = 0, val = 0; // moved interior, moved border, locked, the largest valence: of this thread's vertices
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
        const u64 k = (u64)(row[i + 1] - row[i]);
        const unsigned int nb = nbord[i], fl = vflag[i];
        const bool locked = (fl & VF_MANY) || (nb != 0u && nb != 2u) || k == 0;
        const int cls = locked ? V_LOCKED : nb == 2u ? V_BORDER : V_INTERIOR;
        const bool moves = !locked && (fl & VF_SPLIT);
        vclass[i] = (uint8_t)(cls | (moves ? V_MOVES : 0));
        lk += locked ? 1 : 0;
        mi += (moves && cls == V_INTERIOR) ? 1 : 0;
        mb += (moves && cls == V_BORDER) ? 1 : 0;
        val = k > val ? k : val;
    }
    mi = wave_sum(mi);
    mb = wave_sum(mb);
    lk = wave_sum(lk);
    val = wave_reduce(val, [](u64 x, u64 y) { return y > x ? y : x; });
    if ((threadIdx.x & 63) == 0) {
        if (mi) atomicAdd(ctr + C_MOVED_INTERIOR, mi);
        if (mb) atomicAdd(ctr + C_MOVED_BORDER, mb);
        if (lk) atomicAdd(ctr + C_LOCKED, lk);
        ctr_max(ctr + C_VALENCE, val);
    }
}

// 1 + the split edges of every face (emid is -1 at every entry of a face with a repeated index); the faces by pattern
__global__ __launch_bounds__(256) void k_sd_count(const int32_t *__restrict__ emid, size_t nf, unsigned int *__restrict__ fcnt, u64 *__restrict__ ctr) {
    u64 pat[4] = {0, 0, 0, 0}; // this thread's faces by pattern (the same strided grid as k_sd_vertex)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nf; i += (size_t)gridDim.x * 256) {
        const int ns = (emid[3 * i] >= 0 ? 1 : 0) + (emid[3 * i + 1] >= 0 ? 1 : 0) + (emid[3 * i + 2] >= 0 ? 1 : 0);
        fcnt[i] = 1u + (unsigned int)ns;
        pat[0] += ns == 0 ? 1 : 0;
        pat[1] += ns == 1 ? 1 : 0;
        pat[2] += ns == 2 ? 1 : 0;
        pat[3] += ns == 3 ? 1 : 0;
    }
    for (int c = 0; c < 4; c++) {
        const u64 x = wave_sum(pat[c]);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(ctr + C_PAT0 + c, x);
    }
}
// the two totals beside the counters, so that one copy brings everything an iteration reads back
__global__ void k_sd_totals(const unsigned int *__restrict__ sflag, const unsigned int *__restrict__ srank, size_t n, const unsigned int *__restrict__ fcnt,
                            const unsigned int *__restrict__ fpos, size_t nf, u64 *__restrict__ ctr) {
    ctr[C_NSPLIT] = (u64)srank[n - 1] + (u64)sflag[n - 1];
    ctr[C_NFOUT] = (u64)fpos[nf - 1] + (u64)fcnt[nf - 1];
}

// ---- the points --------------------------------------------------------------------------------------------------------------------------------
// odd: edge (a, b), a < b.  In exactly two faces, with c, d opposite it in the run's order: ((Pa + Pb) 3/8) + ((Pc + Pd) 1/8); else the midpoint
__global__ __launch_bounds__(256) void k_sd_odd(const u64 *__restrict__ key, const uint32_t *__restrict__ val, size_t n, const uint32_t *__restrict__ slist, size_t nsplit,
                                                const float *__restrict__ v, size_t nv, const int32_t *__restrict__ f, float *__restrict__ out) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= nsplit) return;
    const size_t i = slist[r];
    const u64 k = key[i];
    const D3 ab = add3(ld3(v, (size_t)(k >> 32)), ld3(v, (size_t)(k & 0xffffffffull)));
    const bool two = i + 1 < n && key[i + 1] == k && !(i + 2 < n && key[i + 2] == k);
    D3 p;
    if (two) {
        const D3 cd = add3(ld3(v, (size_t)opposite(f, val[i])), ld3(v, (size_t)opposite(f, val[i + 1])));
        p = add3(mul3(ab, 0.375), mul3(cd, 0.125));
    } else {
        p = mul3(ab, 0.5);
    }
    st3(out, nv + r, p);
}

// even: a vertex that does not move keeps its bits.  Interior, k corners: S over the corner list, ascending, per corner the next and then
// the previous vertex; P (1 - k beta_k) + (S / 2) beta_k.  Border, neighbours p, q along the border: P 3/4 + (Pp + Pq) 1/8.
__global__ __launch_bounds__(256) void k_sd_even(const float *__restrict__ v, size_t nv, const int32_t *__restrict__ f, const uint32_t *__restrict__ row,
                                                 const uint32_t *__restrict__ corner, const uint8_t *__restrict__ vclass, const unsigned int *__restrict__ bmin,
                                                 const unsigned int *__restrict__ bsum, const double *__restrict__ beta, float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int c = vclass[i];
    if (!(c & V_MOVES)) {
        for (int a = 0; a < 3; a++) out[3 * i + a] = v[3 * i + a];
        return;
    }
    const D3 p = ld3(v, i);
    if ((c & 3) == V_BORDER) {
        const unsigned int q0 = bmin[i], q1 = bsum[i] - q0;
        st3(out, i, add3(mul3(p, 0.75), mul3(add3(ld3(v, q0), ld3(v, q1)), 0.125)));
        return;
    }
    const uint32_t r0 = row[i], r1 = row[i + 1];
    D3 S = D3{0.0, 0.0, 0.0};
    for (uint32_t r = r0; r < r1; r++) {
        const uint32_t e = corner[r];
        const size_t fi = e / 3;
        const int j = (int)(e % 3);
        S = add3(S, ld3(v, (size_t)f[3 * fi + (j + 1) % 3]));
        S = add3(S, ld3(v, (size_t)f[3 * fi + (j + 2) % 3]));
    }
    const double kd = (double)(r1 - r0), b = beta[r1 - r0];
    st3(out, i, add3(mul3(p, 1.0 - kd * b), mul3(mul3(S, 0.5), b)));
}

// ---- the faces ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void face3(int32_t *__restrict__ out, size_t o, int a, int b, int c) {
    out[3 * o] = a;
    out[3 * o + 1] = b;
    out[3 * o + 2] = c;
}
// face i becomes the faces fpos[i] .. of the result; m_j = emid[3 i + j], the new vertex on edge j = (v_j, v_j+1); vout: this iteration's
// positions (the two-split quad is cut along the shorter of its diagonals there)
__global__ __launch_bounds__(256) void k_sd_emit(const int32_t *__restrict__ f, size_t nf, const int32_t *__restrict__ emid, const unsigned int *__restrict__ fpos,
                                                 const float *__restrict__ vout, int32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nf) return;
    const int v[3] = {f[3 * i], f[3 * i + 1], f[3 * i + 2]};
    const int m[3] = {emid[3 * i], emid[3 * i + 1], emid[3 * i + 2]};
    const int ns = (m[0] >= 0 ? 1 : 0) + (m[1] >= 0 ? 1 : 0) + (m[2] >= 0 ? 1 : 0);
    const size_t o = fpos[i];
    if (ns == 0) {
        face3(out, o, v[0], v[1], v[2]);
    } else if (ns == 3) {
        face3(out, o, v[0], m[0], m[2]);
        face3(out, o + 1, m[0], v[1], m[1]);
        face3(out, o + 2, m[2], m[1], v[2]);
        face3(out, o + 3, m[0], m[1], m[2]);
    } else if (ns == 1) {
        const int j = m[0] >= 0 ? 0 : m[1] >= 0 ? 1 : 2;
        const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        face3(out, o, v[j], m[j], v[j2]);
        face3(out, o + 1, m[j], v[j1], v[j2]);
    } else {
        const int u = m[0] < 0 ? 0 : m[1] < 0 ? 1 : 2; // the edge that stays; j and j + 1 split
        const int j = (u + 1) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        face3(out, o, m[j], v[j1], m[j1]);
        const double from_v = dist2(ld3(vout, (size_t)v[j]), ld3(vout, (size_t)m[j1])), from_m = dist2(ld3(vout, (size_t)m[j]), ld3(vout, (size_t)v[j2]));
        if (from_v <= from_m) {
            face3(out, o + 1, v[j], m[j], m[j1]);
            face3(out, o + 2, v[j], m[j1], v[j2]);
        } else {
            face3(out, o + 1, v[j], m[j], v[j2]);
            face3(out, o + 2, m[j], m[j1], v[j2]);
        }
    }
}

// ---- the stage entry's view of one iteration: the unique edges in key order ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sd_heads(const u64 *__restrict__ key, size_t n, u64 nv, unsigned int *__restrict__ head) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = key[i];
    head[i] = ((k >> 32) != nv && (i == 0 || key[i - 1] != k)) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_sd_unique(const u64 *__restrict__ key, size_t n, const unsigned int *__restrict__ head, const unsigned int *__restrict__ upos,
                                                   const unsigned int *__restrict__ sflag, const unsigned int *__restrict__ srank, const float *__restrict__ vout, size_t nv,
                                                   u64 *__restrict__ ukey, int32_t *__restrict__ mult, int32_t *__restrict__ split, float *__restrict__ pos) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !head[i]) return;
    const u64 k = key[i];
    int m = 1;
    while (i + m < n && key[i + m] == k) m++;
    const size_t e = upos[i];
    ukey[e] = k;
    mult[e] = m;
    split[e] = (int32_t)sflag[i];
    for (int a = 0; a < 3; a++) pos[3 * e + a] = sflag[i] ? vout[3 * (nv + srank[i]) + a] : 0.0f;
}
__global__ __launch_bounds__(256) void k_sd_class(const uint8_t *__restrict__ vclass, size_t nv, int32_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nv) out[i] = (int32_t)(vclass[i] & 3);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
// beta_k = (5/8 - (3/8 + cos(2 pi / k) / 4)^2) / k, in fp64 with the C library's cos (the restatement's math.cos is the same function),
// k = 1 .. the largest valence met; on the device as a table.  BETA_ROOM entries are allocated before the first launch; a vertex in more
// faces than that costs the call one allocation behind a read-back.
#define BETA_ROOM 4096
struct BetaTable {
    std::vector<double> h;
    double *d = nullptr;
    size_t room = 0, up = 0; // entries allocated / uploaded
    int ensure(DevMem &M, size_t kmax, hipStream_t st) {
        if (kmax < up) return RSM_OK;
        if (kmax >= room) {
            room = kmax + 1;
            up = 0;
            if (!(d = M.get<double>(room))) return RSM_E_NOMEM;
        }
        const double two_pi = 2.0 * M_PI;
        if (h.empty()) h.push_back(0.0);
        for (size_t k = h.size(); k <= kmax; k++) {
            const double t = 0.375 + 0.25 * cos(two_pi / (double)k);
            h.push_back((0.625 - t * t) / (double)k);
        }
        // (the whole table again: the copy is small and h may have moved.  Called behind a read-back, so no earlier copy still reads h; the
        // table is declared in front of the call's scratch and so outlives everything on the stream)
        DEVCHK(hipMemcpyAsync(d, h.data(), (kmax + 1) * sizeof(double), hipMemcpyHostToDevice, st));
        up = kmax + 1;
        return RSM_OK;
    }
};

#define COUNT_BLOCKS 1024
static inline dim3 count_blocks(size_t n) { return dim3((unsigned)std::min<size_t>((n + 255) / 256, COUNT_BLOCKS)); }

// an iteration's scratch from one allocation: 40 bytes a corner of its own, 16 for the corner lists, the two sorts' temporaries
static size_t pool_bytes(size_t nv, size_t nf) { return 120 * 3 * nf + 40 * nv + ((size_t)1 << 20); }

struct Iter { // one iteration's tables, and what it read back
    size_t nv = 0, nf = 0;
    const float *V = nullptr;
    const int32_t *F = nullptr;
    u64 *ekey = nullptr, *ctr = nullptr;
    uint32_t *eval = nullptr, *row = nullptr, *corner = nullptr, *slist = nullptr;
    unsigned int *sflag = nullptr, *srank = nullptr, *fcnt = nullptr, *fpos = nullptr, *nbord = nullptr, *vflag = nullptr, *bmin = nullptr, *bsum = nullptr;
    int32_t *emid = nullptr;
    uint8_t *vclass = nullptr;
    u64 h[C_N] = {0};
};

// everything of an iteration up to its read-back; nv > 0, nf > 0, a validated mesh.  Allocates, then enqueues.
static int iter_count(Pool &M, Iter &T, const float *V, size_t nv, const int32_t *F, size_t nf, double thr2, hipStream_t st) {
    const size_t n = 3 * nf;
    T.nv = nv, T.nf = nf, T.V = V, T.F = F;
    u64 *k0 = M.get<u64>(n);
    uint32_t *v0 = M.get<uint32_t>(n);
    T.ekey = M.get<u64>(n);
    T.eval = M.get<uint32_t>(n);
    T.sflag = M.get<unsigned int>(n);
    T.srank = M.get<unsigned int>(n);
    T.slist = M.get<uint32_t>(n);
    T.emid = M.get<int32_t>(n);
    T.fcnt = M.get<unsigned int>(nf);
    T.fpos = M.get<unsigned int>(nf);
    T.nbord = M.get<unsigned int>(nv);
    T.vflag = M.get<unsigned int>(nv);
    T.bmin = M.get<unsigned int>(nv);
    T.bsum = M.get<unsigned int>(nv);
    T.vclass = M.get<uint8_t>(nv);
    T.ctr = M.get<u64>(C_N);
    // (the scans' temporaries: rocprim sizes them without touching the stream)
    size_t tb_e = 0, tb_f = 0;
    DEVCHK(rocprim::exclusive_scan(nullptr, tb_e, (const unsigned int *)T.sflag, T.srank, 0u, n, rocprim::plus<unsigned int>(), st));
    DEVCHK(rocprim::exclusive_scan(nullptr, tb_f, (const unsigned int *)T.fcnt, T.fpos, 0u, nf, rocprim::plus<unsigned int>(), st));
    ScanTmp te, tf;
    te.bytes = tb_e, tf.bytes = tb_f;
    te.p = M.get<uint8_t>(tb_e);
    tf.p = M.get<uint8_t>(tb_f);
    if (!k0 || !v0 || !T.ekey || !T.eval || !T.sflag || !T.srank || !T.slist || !T.emid || !T.fcnt || !T.fpos || !T.nbord || !T.vflag || !T.bmin || !T.bsum ||
        !T.vclass || !T.ctr || !te.p || !tf.p)
        return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(T.ctr, 0, C_N * sizeof(u64), st));
    DEVCHK(hipMemsetAsync(T.nbord, 0, nv * sizeof(unsigned int), st));
    DEVCHK(hipMemsetAsync(T.vflag, 0, nv * sizeof(unsigned int), st));
    DEVCHK(hipMemsetAsync(T.bsum, 0, nv * sizeof(unsigned int), st));
    DEVCHK(hipMemsetAsync(T.bmin, 0xff, nv * sizeof(unsigned int), st));
    DEVCHK(hipMemsetAsync(T.emid, 0xff, n * sizeof(int32_t), st));
    int s = mesh_edge_table(M, F, nv, nf, k0, v0, T.ekey, T.eval, st);
    if (s != RSM_OK || (s = mesh_corner_lists(M, F, nv, nf, &T.row, &T.corner, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_sd_edges, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, n, (u64)nv, V, thr2, T.sflag, T.nbord, T.vflag, T.bmin, T.bsum, T.ctr);
    if ((s = scan_u32(M, (const unsigned int *)T.sflag, T.srank, n, st, &te)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_sd_marks, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, (const uint32_t *)T.eval, n, (u64)nv, (const unsigned int *)T.sflag,
                       (const unsigned int *)T.srank, T.slist, T.emid);
    hipLaunchKernelGGL(k_sd_vertex, count_blocks(nv), dim3(256), 0, st, nv, (const uint32_t *)T.row, (const unsigned int *)T.nbord, (const unsigned int *)T.vflag, T.vclass,
                       T.ctr);
    hipLaunchKernelGGL(k_sd_count, count_blocks(nf), dim3(256), 0, st, (const int32_t *)T.emid, nf, T.fcnt, T.ctr);
    if ((s = scan_u32(M, (const unsigned int *)T.fcnt, T.fpos, nf, st, &tf)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_sd_totals, dim3(1), dim3(1), 0, st, (const unsigned int *)T.sflag, (const unsigned int *)T.srank, n, (const unsigned int *)T.fcnt,
                       (const unsigned int *)T.fpos, nf, T.ctr);
    DEVCHK(hipMemcpyAsync(T.h, T.ctr, C_N * sizeof(u64), hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st)); // the iteration's one read-back
    return RSM_OK;
}

// the iteration's result into Vout (room for nv + split vertices) and Fout (room for the counted faces); enqueues only
static void iter_emit(const Iter &T, const double *d_beta, float *Vout, int32_t *Fout, hipStream_t st) {
    const size_t n = 3 * T.nf, nsplit = (size_t)T.h[C_NSPLIT];
    if (nsplit > 0)
        hipLaunchKernelGGL(k_sd_odd, blocks_for(nsplit), dim3(256), 0, st, (const u64 *)T.ekey, (const uint32_t *)T.eval, n, (const uint32_t *)T.slist, nsplit, T.V, T.nv,
                           T.F, Vout);
    hipLaunchKernelGGL(k_sd_even, blocks_for(T.nv), dim3(256), 0, st, T.V, T.nv, T.F, (const uint32_t *)T.row, (const uint32_t *)T.corner, (const uint8_t *)T.vclass,
                       (const unsigned int *)T.bmin, (const unsigned int *)T.bsum, d_beta, Vout);
    hipLaunchKernelGGL(k_sd_emit, blocks_for(T.nf), dim3(256), 0, st, T.F, T.nf, (const int32_t *)T.emid, (const unsigned int *)T.fpos, (const float *)Vout, Fout);
}

// thr of a call: the absolute threshold, or the fraction of the fp64 diagonal of the vertices' float32 box (one read-back; no vertex: 0)
static int call_threshold(DevMem &M, const float *d_v, size_t nv, const rsm_mesh_subdivide_params *p, double *thr, hipStream_t st) {
    *thr = p->threshold;
    if (!(p->threshold_fraction > 0.0)) return RSM_OK;
    *thr = 0.0;
    if (nv == 0) return RSM_OK;
    unsigned int *mm = M.get<unsigned int>(6);
    if (!mm) return RSM_E_NOMEM;
    unsigned int h[6];
    DEVCHK(hipMemsetAsync(mm, 0xff, 3 * sizeof(unsigned int), st));
    DEVCHK(hipMemsetAsync(mm + 3, 0, 3 * sizeof(unsigned int), st));
    const size_t blocks = (nv + 255) / 256;
    hipLaunchKernelGGL(k_mesh_vertex_box<>, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, d_v, nv, mm);
    DEVCHK(hipMemcpyAsync(h, mm, sizeof h, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    *thr = p->threshold_fraction * sqrt(box_diagonal2(h));
    return RSM_OK;
}

// the result buffers a call made: all but the one it hands out go at its end
struct Made {
    std::vector<PoissonMesh> m;
    ~Made() {
        for (PoissonMesh &x : m) poisson_mesh_free(&x);
    }
};

} // namespace

int mesh_subdivide_edges_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const rsm_mesh_subdivide_params *p, uint64_t *d_key, int32_t *d_mult,
                                int32_t *d_split, float *d_odd, int64_t *n_edges, int32_t *d_class, float *d_even, double *thr_used, int *invalid, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_, n = 3 * nf;
    *n_edges = 0;
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK) return s;
    BetaTable B;
    DevMem M;
    double thr = 0.0;
    if ((s = call_threshold(M, d_v, nv, p, &thr, st)) != RSM_OK) return s;
    if (thr_used) *thr_used = thr;
    if (nv == 0) return RSM_OK;
    if (nf == 0) { // vertices in no face: locked, where they are
        uint8_t *two = M.get<uint8_t>(nv);
        if (!two) return RSM_E_NOMEM;
        DEVCHK(hipMemsetAsync(two, V_LOCKED, nv, st));
        hipLaunchKernelGGL(k_sd_class, blocks_for(nv), dim3(256), 0, st, (const uint8_t *)two, nv, d_class);
        DEVCHK(hipMemcpyAsync(d_even, d_v, 3 * nv * sizeof(float), hipMemcpyDeviceToDevice, st));
        return mesh_finish(st);
    }
    unsigned int *head = M.get<unsigned int>(n), *upos = M.get<unsigned int>(n);
    double *beta0 = M.get<double>(BETA_ROOM);
    if (!M.ok) return RSM_E_NOMEM;
    Pool R(pool_bytes(nv, nf));
    Iter T;
    if ((s = iter_count(R, T, d_v, nv, d_f, nf, thr * thr, st)) != RSM_OK) return s;
    if (!subdivide_sizes_ok(nv, T.h[C_NSPLIT], T.h[C_NFOUT])) {
        *invalid = MESH_INVALID_TOO_LARGE;
        return RSM_E_INVALID;
    }
    const size_t nsplit = (size_t)T.h[C_NSPLIT];
    float *Vout = M.get<float>(3 * (nv + nsplit));
    int32_t *Fout = M.get<int32_t>(3 * (size_t)T.h[C_NFOUT]);
    if (!M.ok) return RSM_E_NOMEM;
    B.d = beta0, B.room = BETA_ROOM;
    if ((s = B.ensure(M, (size_t)T.h[C_VALENCE], st)) != RSM_OK) return s;
    iter_emit(T, B.d, Vout, Fout, st);
    hipLaunchKernelGGL(k_sd_heads, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, n, (u64)nv, head);
    if ((s = scan_u32(M, (const unsigned int *)head, upos, n, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_sd_unique, blocks_for(n), dim3(256), 0, st, (const u64 *)T.ekey, n, (const unsigned int *)head, (const unsigned int *)upos,
                       (const unsigned int *)T.sflag, (const unsigned int *)T.srank, (const float *)Vout, nv, (u64 *)d_key, d_mult, d_split, d_odd);
    hipLaunchKernelGGL(k_sd_class, blocks_for(nv), dim3(256), 0, st, (const uint8_t *)T.vclass, nv, d_class);
    DEVCHK(hipMemcpyAsync(d_even, Vout, 3 * nv * sizeof(float), hipMemcpyDeviceToDevice, st));
    uint64_t ne = 0;
    if ((s = scan_total(head, upos, n, st, &ne)) != RSM_OK) return s;
    *n_edges = (int64_t)ne;
    return mesh_finish(st);
}

int mesh_subdivide_device(const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const rsm_mesh_subdivide_params *p, PoissonMesh *out, double *stats, int *invalid,
                          hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    double S[RSM_MESH_SUBDIVIDE_STATS] = {0};
    S[0] = (double)nv;
    S[1] = (double)nf;
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK) return s;
    BetaTable B;
    DevMem M;
    std::vector<std::unique_ptr<Pool>> pools; // the scratch of every iteration, one allocation each: nothing is freed while work is on the stream
    Made made;
    double thr = 0.0;
    if ((s = call_threshold(M, d_v, nv, p, &thr, st)) != RSM_OK) return s;
    S[5] = thr;
    const float *V = d_v;
    const int32_t *F = d_f;
    size_t cnv = nv, cnf = nf;
    int done = 0;
    if (nv > 0 && nf > 0) {
        B.room = BETA_ROOM;
        if (!(B.d = M.get<double>(BETA_ROOM))) return RSM_E_NOMEM;
        for (int it = 0; it < p->iterations; it++) {
            Iter T;
            pools.emplace_back(new Pool(pool_bytes(cnv, cnf)));
            if ((s = iter_count(*pools.back(), T, V, cnv, F, cnf, thr * thr, st)) != RSM_OK) return s;
            S[15] = (double)T.h[C_LOCKED];
            if ((double)T.h[C_VALENCE] > S[16]) S[16] = (double)T.h[C_VALENCE];
            if (T.h[C_NSPLIT] == 0) break; // nothing left to split: the call ends
            if (!subdivide_sizes_ok(cnv, T.h[C_NSPLIT], T.h[C_NFOUT])) {
                *invalid = MESH_INVALID_TOO_LARGE + it;
                return RSM_E_INVALID;
            }
            made.m.emplace_back();
            PoissonMesh &R = made.m.back();
            if ((s = mesh_result_alloc(R, cnv + (size_t)T.h[C_NSPLIT], (size_t)T.h[C_NFOUT])) != RSM_OK) return s;
            if ((s = B.ensure(M, (size_t)T.h[C_VALENCE], st)) != RSM_OK) return s;
            iter_emit(T, B.d, R.d_v, R.d_f, st);
            S[6] += (double)T.h[C_NSPLIT];
            S[7] += (double)T.h[C_SPLIT_BORDER];
            S[8] += (double)T.h[C_SPLIT_MANY];
            for (int c = 0; c < 4; c++) S[9 + c] += (double)T.h[C_PAT0 + c];
            S[13] += (double)T.h[C_MOVED_INTERIOR];
            S[14] += (double)T.h[C_MOVED_BORDER];
            V = R.d_v, F = R.d_f, cnv = (size_t)R.nv, cnf = (size_t)R.nf;
            done++;
        }
    }
    if (done == 0) { // the input as it is
        made.m.emplace_back();
        PoissonMesh &R = made.m.back();
        if ((s = mesh_result_alloc(R, nv, nf)) != RSM_OK) return s;
        if (nv > 0) DEVCHK(hipMemcpyAsync(R.d_v, d_v, 3 * nv * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (nf > 0) DEVCHK(hipMemcpyAsync(R.d_f, d_f, 3 * nf * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
    if ((s = mesh_finish(st)) != RSM_OK) return s;
    const PoissonMesh res = made.m.back();
    made.m.pop_back();
    S[2] = (double)res.nv;
    S[3] = (double)res.nf;
    S[4] = (double)done;
    if (stats) memcpy(stats, S, sizeof S);
    mesh_result_commit(out, res);
    return RSM_OK;
}
