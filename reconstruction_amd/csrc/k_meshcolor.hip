// k_meshcolor.hip -- colours of the final mesh from the rig's views, where CCloudOptimization::run hands bigmesh.ply and scans.txt to
// TextureStitcher (CCloudOptimization.cpp:394-397).  Not a bit-parity port of that tool (no source in the
// reference tree): every rule is defined in DESIGN.md 9 (f9) and restated in numpy in tests/meshcolor_restatement.py, and the kernels are
// held to that restatement exactly.  The one part with source, texture_color (:400-421), is restated literally.
//   texture_color  q = R p + T (float, project_common.h), pixel = ROUND of the float quotients, (127, 127, 127) outside the image or where
//                  the reference is undefined, else the BGR pixel as RGB; no test of q2's sign                     k_mcol_texture
//   depth buffer   per view W x H uint32 = the largest float32 bit pattern of the inverse depth drawn at each pixel centre: integer
//                  atomicMax, whose result does not depend on the order of arrival.  One thread per (face, view) walks the face's
//                  bounding box; a box of more than `big_box` pixels goes to a list that one block per item strides -- the same pixels
//                  and values in both tiers                                                                     k_mcol_raster, k_mcol_raster_big
//   colours        one thread per vertex: the normal by a gather through the corner lists of k_meshclean.hip (ascending 3 f + j, fp64),
//                  then the views in order: visibility, the best view, the cos-weighted blend                     k_mcol_color
// No float atomics; every sum is a gather in a fixed order.  Built with -ffp-contract=off (csrc/Makefile): every expression below is
// evaluated as written.
#include "../../include/rsm.h"
#include "rsm_dev.h"
#include "meshcolor_common.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace {

typedef unsigned long long u64;

enum { K_COLOURED = 0, K_NONORMAL, K_VISIBLE, K_DRAWN, K_BIG, K_CURSOR, K_N };

__device__ __forceinline__ void count_if(bool flag, u64 *ctr) {
    if (flag) atomicAdd(ctr, (u64)1);
}

// ---- texture_color over an array ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mcol_texture(const float *__restrict__ p, size_t n, McView c, uint8_t *__restrict__ rgb) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float q0, q1, q2;
    mcol_q(c, p[3 * i], p[3 * i + 1], p[3 * i + 2], &q0, &q1, &q2);
    size_t pix;
    uint8_t r = 127, g = 127, b = 127;
    if (mcol_pixel(q0, q1, q2, c.W, c.H, &pix)) {
        b = c.img[3 * pix];
        g = c.img[3 * pix + 1];
        r = c.img[3 * pix + 2];
    }
    rgb[3 * i] = r;
    rgb[3 * i + 1] = g;
    rgb[3 * i + 2] = b;
}

// ---- the depth buffer ---------------------------------------------------------------------------------------------------------------
struct McTri {
    double u[3], v[3], w[3], A;
    int x0, x1, y0, y1; // the bounding box inside the image, inclusive
};

// E(a, b, p) = (bu - au)(pv - av) - (bv - av)(pu - au)
__device__ __forceinline__ double mcol_edge(double au, double av, double bu, double bv, double pu, double pv) { return (bu - au) * (pv - av) - (bv - av) * (pu - au); }

__device__ __forceinline__ double min3(double a, double b, double c) {
    const double m = a < b ? a : b;
    return m < c ? m : c;
}
__device__ __forceinline__ double max3(double a, double b, double c) {
    const double m = a > b ? a : b;
    return m > c ? m : c;
}

// face fi in view c: false when it draws nothing (a vertex with q2 <= 0 or a quotient that is not finite, no area, a box outside the image)
__device__ __forceinline__ bool mcol_tri(const McView &c, const float *__restrict__ p, const int32_t *__restrict__ f, size_t fi, McTri *t) {
    for (int k = 0; k < 3; k++) {
        const size_t vi = (size_t)f[3 * fi + k];
        float q0, q1, q2;
        mcol_q(c, p[3 * vi], p[3 * vi + 1], p[3 * vi + 2], &q0, &q1, &q2);
        if (!(q2 > 0.0f)) return false;
        const float uf = q0 / q2, vf = q1 / q2;
        if (!isfinite(uf) || !isfinite(vf)) return false;
        t->u[k] = (double)uf;
        t->v[k] = (double)vf;
        t->w[k] = 1.0 / (double)q2;
    }
    t->A = mcol_edge(t->u[0], t->v[0], t->u[1], t->v[1], t->u[2], t->v[2]);
    if (t->A == 0.0) return false;
    double x0 = ceil(min3(t->u[0], t->u[1], t->u[2])), x1 = floor(max3(t->u[0], t->u[1], t->u[2]));
    double y0 = ceil(min3(t->v[0], t->v[1], t->v[2])), y1 = floor(max3(t->v[0], t->v[1], t->v[2]));
    x0 = x0 < 0.0 ? 0.0 : x0;
    y0 = y0 < 0.0 ? 0.0 : y0;
    x1 = x1 > (double)(c.W - 1) ? (double)(c.W - 1) : x1;
    y1 = y1 > (double)(c.H - 1) ? (double)(c.H - 1) : y1;
    if (x0 > x1 || y0 > y1) return false;
    t->x0 = (int)x0; // (all four lie in [0, W - 1] x [0, H - 1] here)
    t->x1 = (int)x1;
    t->y0 = (int)y0;
    t->y1 = (int)y1;
    return true;
}

// pixel centre (x, y) of the box: inside all three edges (inclusive, either orientation) -> max of the inverse depth's float bits
__device__ __forceinline__ void mcol_draw(const McView &c, const McTri &t, int x, int y) {
    const double pu = (double)x, pv = (double)y;
    const double e0 = mcol_edge(t.u[1], t.v[1], t.u[2], t.v[2], pu, pv);
    const double e1 = mcol_edge(t.u[2], t.v[2], t.u[0], t.v[0], pu, pv);
    const double e2 = mcol_edge(t.u[0], t.v[0], t.u[1], t.v[1], pu, pv);
    const double s = t.A > 0.0 ? 1.0 : -1.0;
    if (!(e0 * s >= 0.0 && e1 * s >= 0.0 && e2 * s >= 0.0)) return;
    const double l0 = e0 / t.A, l1 = e1 / t.A, l2 = e2 / t.A;
    const double w = (l0 * t.w[0] + l1 * t.w[1]) + l2 * t.w[2];
    const uint32_t bits = __float_as_uint((float)w);
    uint32_t *dst = c.wbuf + ((size_t)y * (size_t)c.W + (size_t)x);
    // (a stale read only costs an atomic that changes nothing)
    if (__hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits) atomicMax(dst, bits);
}

// one thread per (face, view): blockIdx.y is the view.  PASS 0 draws the boxes of at most big_box pixels and counts the others;
// PASS 1 lists the others (face, view) for k_mcol_raster_big.
template <int PASS>
__global__ __launch_bounds__(256) void k_mcol_raster(const float *__restrict__ p, const int32_t *__restrict__ f, size_t nf, const McView *__restrict__ views,
                                                     long long big_box, uint2 *__restrict__ list, u64 n_list, u64 *__restrict__ ctr) {
    const size_t fi = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool drawn = false, big = false;
    if (fi < nf) {
        const McView &c = views[blockIdx.y];
        McTri t;
        if (mcol_tri(c, p, f, fi, &t)) {
            drawn = true;
            big = (long long)(t.x1 - t.x0 + 1) * (long long)(t.y1 - t.y0 + 1) > big_box;
            if (PASS == 0 && !big) {
                for (int y = t.y0; y <= t.y1; y++)
                    for (int x = t.x0; x <= t.x1; x++) mcol_draw(c, t, x, y);
            }
            if (PASS == 1 && big) {
                const u64 k = atomicAdd(ctr + K_CURSOR, (u64)1);
                if (k < n_list) list[k] = make_uint2((unsigned)fi, blockIdx.y);
            }
        }
    }
    if (PASS == 0) {
        count_if(drawn, ctr + K_DRAWN);
        count_if(big, ctr + K_BIG);
    }
}

// one block per listed item strides its box
__global__ __launch_bounds__(256) void k_mcol_raster_big(const float *__restrict__ p, const int32_t *__restrict__ f, const McView *__restrict__ views,
                                                         const uint2 *__restrict__ list) {
    const uint2 item = list[blockIdx.x];
    const McView &c = views[item.y];
    McTri t;
    if (!mcol_tri(c, p, f, (size_t)item.x, &t)) return;
    const size_t bw = (size_t)(t.x1 - t.x0 + 1), n = bw * (size_t)(t.y1 - t.y0 + 1);
    for (size_t i = threadIdx.x; i < n; i += 256) mcol_draw(c, t, t.x0 + (int)(i % bw), t.y0 + (int)(i / bw));
}

// ---- colours ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mcol_color(const float *__restrict__ p, size_t nv, const int32_t *__restrict__ f, const uint32_t *__restrict__ row,
                                                    const uint32_t *__restrict__ corner, const McView *__restrict__ views, int V, int mode, double min_cos,
                                                    double depth_eps, uint8_t *__restrict__ rgb, int32_t *__restrict__ best_view, u64 *__restrict__ vis, u64 *__restrict__ ctr) {
    const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool coloured = false, no_normal = false;
    u64 n_vis = 0, seen = 0; // seen: bit k = view k sees the vertex (written only where vis is given: V <= 64 there)
    if (j < nv) {
        // the normal: the faces' (P1 - P0) x (P2 - P0), fp64 from the float positions, summed over the corner list in ascending 3 f + j
        double nx = 0.0, ny = 0.0, nz = 0.0;
        for (uint32_t r = row[j]; r < row[j + 1]; r++) {
            const size_t fi = corner[r] / 3;
            const size_t a = (size_t)f[3 * fi], b = (size_t)f[3 * fi + 1], c = (size_t)f[3 * fi + 2];
            const double ax = (double)p[3 * a], ay = (double)p[3 * a + 1], az = (double)p[3 * a + 2];
            const double u0 = (double)p[3 * b] - ax, u1 = (double)p[3 * b + 1] - ay, u2 = (double)p[3 * b + 2] - az;
            const double w0 = (double)p[3 * c] - ax, w1 = (double)p[3 * c + 1] - ay, w2 = (double)p[3 * c + 2] - az;
            nx += u1 * w2 - u2 * w1;
            ny += u2 * w0 - u0 * w2;
            nz += u0 * w1 - u1 * w0;
        }
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        int best = -1;
        double best_cos = 0.0, sw = 0.0, sr = 0.0, sg = 0.0, sb = 0.0;
        uint8_t br = 127, bg = 127, bb = 127;
        if (!(len > 0.0)) no_normal = true;
        else {
            nx = nx / len;
            ny = ny / len;
            nz = nz / len;
            const float px = p[3 * j], py = p[3 * j + 1], pz = p[3 * j + 2];
            for (int k = 0; k < V; k++) {
                const McView &c = views[k];
                float q0, q1, q2;
                mcol_q(c, px, py, pz, &q0, &q1, &q2);
                if (!(q2 > 0.0f)) continue;
                size_t pix;
                if (!mcol_pixel(q0, q1, q2, c.W, c.H, &pix)) continue;
                if (c.mask && c.mask[pix] != 255) continue;
                const double d0 = c.C[0] - (double)px, d1 = c.C[1] - (double)py, d2 = c.C[2] - (double)pz;
                const double cs = ((nx * d0 + ny * d1) + nz * d2) / sqrt((d0 * d0 + d1 * d1) + d2 * d2);
                if (!(cs > min_cos)) continue;
                const uint32_t wb = c.wbuf[pix];
                if (wb != 0 && !((double)q2 <= 1.0 / (double)__uint_as_float(wb) + depth_eps)) continue;
                n_vis++;
                seen |= (u64)1 << (k & 63);
                const uint8_t cb = c.img[3 * pix], cg = c.img[3 * pix + 1], cr = c.img[3 * pix + 2];
                if (best < 0 || cs > best_cos) { // (strict: a tie stays with the lower view)
                    best = k;
                    best_cos = cs;
                    br = cr;
                    bg = cg;
                    bb = cb;
                }
                const double w = cs > 0.0 ? cs : 0.0; // (min_cos < 0 lets a view in that faces away: it carries no weight)
                sw += w;
                sr += w * (double)cr;
                sg += w * (double)cg;
                sb += w * (double)cb;
            }
        }
        coloured = best >= 0;
        if (coloured && mode == 1 && sw > 0.0) {
            br = (uint8_t)(int)(sr / sw + 0.5);
            bg = (uint8_t)(int)(sg / sw + 0.5);
            bb = (uint8_t)(int)(sb / sw + 0.5);
        }
        rgb[3 * j] = br;
        rgb[3 * j + 1] = bg;
        rgb[3 * j + 2] = bb;
        if (best_view) best_view[j] = best;
        if (vis) vis[j] = seen;
    }
    count_if(coloured, ctr + K_COLOURED);
    count_if(no_normal, ctr + K_NONORMAL);
    if (n_vis) atomicAdd(ctr + K_VISIBLE, n_vis);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// the determinant of the matrix whose columns are a, b, c, expanded along the first column
static double det3(const double a[3], const double b[3], const double c[3]) {
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// R, T = the float casts of P's columns; with_center: C = -M^-1 p4 by Cramer's rule in fp64, false when det M = 0
static bool view_from_P(const double P[12], bool with_center, McView *c) {
    double col[4][3];
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) c->R[3 * r + k] = (float)P[4 * r + k];
        c->T[r] = (float)P[4 * r + 3];
        for (int k = 0; k < 4; k++) col[k][r] = P[4 * r + k];
    }
    c->C[0] = c->C[1] = c->C[2] = 0.0;
    if (!with_center) return true;
    const double det = det3(col[0], col[1], col[2]);
    if (det == 0.0 || !std::isfinite(det)) return false;
    c->C[0] = -(det3(col[3], col[1], col[2]) / det);
    c->C[1] = -(det3(col[0], col[3], col[2]) / det);
    c->C[2] = -(det3(col[0], col[1], col[3]) / det);
    return true;
}

// the depth buffers of V views (cleared here); ctr[K_DRAWN] / ctr[K_BIG] count the items.  One host round trip (the size of the list).
static int raster(DevMem &M, const float *d_v, const int32_t *d_f, size_t nf, const std::vector<McView> &hv, const McView *d_views, long long big_box, u64 *ctr,
                  hipStream_t st) {
    const int V = (int)hv.size();
    for (const McView &c : hv) DEVCHK(hipMemsetAsync(c.wbuf, 0, sizeof(uint32_t) * (size_t)c.W * (size_t)c.H, st));
    if (nf == 0) return RSM_OK;
    const dim3 grid(blocks_for(nf).x, (unsigned)V);
    hipLaunchKernelGGL(k_mcol_raster<0>, grid, dim3(256), 0, st, d_v, d_f, nf, d_views, big_box, (uint2 *)nullptr, (u64)0, ctr);
    u64 n_big = 0;
    DEVCHK(hipMemcpyAsync(&n_big, ctr + K_BIG, sizeof n_big, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    if (n_big == 0) return RSM_OK;
    if (n_big > 0x7fffffffull) return RSM_E_NOMEM;
    uint2 *list = M.get<uint2>((size_t)n_big);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(list, 0, sizeof(uint2) * (size_t)n_big, st));
    hipLaunchKernelGGL(k_mcol_raster<1>, grid, dim3(256), 0, st, d_v, d_f, nf, d_views, big_box, list, n_big, ctr);
    hipLaunchKernelGGL(k_mcol_raster_big, dim3((unsigned)n_big), dim3(256), 0, st, d_v, d_f, d_views, (const uint2 *)list);
    return RSM_OK;
}

} // namespace

int texture_color_device(const float *d_xyz, int64_t n, const double P12[12], const uint8_t *d_img, int W, int H, uint8_t *d_rgb, hipStream_t st) {
    if (n <= 0) return RSM_OK;
    McView c;
    memset(&c, 0, sizeof c);
    view_from_P(P12, false, &c);
    c.W = W;
    c.H = H;
    c.img = d_img;
    hipLaunchKernelGGL(k_mcol_texture, blocks_for((size_t)n), dim3(256), 0, st, d_xyz, (size_t)n, c, d_rgb);
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    return RSM_OK;
}

int mesh_depth_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const double P12[12], int W, int H, long long big_box, uint32_t *d_wbuf,
                      int *invalid, hipStream_t st) {
    int s = mesh_validate_device(d_v, nv, d_f, nf, invalid, st);
    if (s != RSM_OK) return s;
    DevMem M;
    std::vector<McView> hv(1);
    memset(&hv[0], 0, sizeof(McView));
    view_from_P(P12, false, &hv[0]);
    hv[0].W = W;
    hv[0].H = H;
    hv[0].wbuf = d_wbuf;
    McView *d_views = M.get<McView>(1);
    u64 *ctr = M.get<u64>(K_N);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemcpyAsync(d_views, hv.data(), sizeof(McView), hipMemcpyHostToDevice, st));
    DEVCHK(hipMemsetAsync(ctr, 0, K_N * sizeof(u64), st));
    if ((s = raster(M, d_v, d_f, (size_t)nf, hv, d_views, big_box, ctr, st)) != RSM_OK) return s;
    DEVCHK(hipStreamSynchronize(st));
    DEVCHK(hipGetLastError());
    return RSM_OK;
}

int mesh_views_device(DevMem &M, const rsm_dedup_view *views, int n_pairs, bool with_wbuf, std::vector<McView> *hv_, McView **d_views, int *invalid, hipStream_t st) {
    // the views in scans.txt's order: every pair's view 0, then every pair's view 1
    const int V = 2 * n_pairs;
    std::vector<McView> &hv = *hv_;
    hv.resize((size_t)V);
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < n_pairs; i++) {
            McView &c = hv[(size_t)k * n_pairs + i];
            memset(&c, 0, sizeof c);
            if (!view_from_P(views[i].P[k], true, &c)) {
                *invalid = 3;
                return RSM_E_INVALID;
            }
            c.W = views[i].width;
            c.H = views[i].height;
        }
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < n_pairs; i++) {
            McView &c = hv[(size_t)k * n_pairs + i];
            const size_t pix = (size_t)c.W * (size_t)c.H;
            uint8_t *img = M.get<uint8_t>(3 * pix), *msk = views[i].mask[k] ? M.get<uint8_t>(pix) : nullptr;
            c.wbuf = with_wbuf ? M.get<uint32_t>(pix) : nullptr;
            if (!M.ok) return RSM_E_NOMEM;
            DEVCHK(hipMemcpyAsync(img, views[i].image[k], 3 * pix, hipMemcpyHostToDevice, st));
            if (msk) DEVCHK(hipMemcpyAsync(msk, views[i].mask[k], pix, hipMemcpyHostToDevice, st));
            c.img = img;
            c.mask = msk;
        }
    *d_views = M.get<McView>((size_t)V);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemcpyAsync(*d_views, hv.data(), sizeof(McView) * (size_t)V, hipMemcpyHostToDevice, st));
    return RSM_OK;
}

int mesh_color_scene_device(DevMem &M, const float *d_v, int64_t nv_, const int32_t *d_f, int64_t nf_, const rsm_dedup_view *views, int n_pairs,
                            const rsm_mesh_color_params *p, long long big_box, uint8_t *d_rgb, int32_t *d_best, u64 *d_vis, double *stats, int *invalid,
                            McScene *scene, hipStream_t st) {
    const size_t nv = (size_t)nv_, nf = (size_t)nf_;
    double S[RSM_MESH_COLOR_STATS] = {0};
    S[0] = (double)nv;
    int s = mesh_validate_device(d_v, nv_, d_f, nf_, invalid, st);
    if (s != RSM_OK) return s;
    if (nv == 0) {
        if (stats) memcpy(stats, S, sizeof S);
        return RSM_OK;
    }
    const int V = 2 * n_pairs;
    std::vector<McView> hv;
    McView *d_views = nullptr;
    if ((s = mesh_views_device(M, views, n_pairs, true, &hv, &d_views, invalid, st)) != RSM_OK) return s;
    u64 *ctr = M.get<u64>(K_N);
    if (!M.ok) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(ctr, 0, K_N * sizeof(u64), st));
    uint32_t *row = nullptr, *corner = nullptr;
    if ((s = mesh_corner_lists(M, d_f, nv, nf, &row, &corner, st)) != RSM_OK) return s;
    if ((s = raster(M, d_v, d_f, nf, hv, d_views, big_box, ctr, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_mcol_color, blocks_for(nv), dim3(256), 0, st, d_v, nv, d_f, (const uint32_t *)row, (const uint32_t *)corner, (const McView *)d_views, V,
                       p->mode, p->min_cos, p->depth_eps, d_rgb, d_best, d_vis, ctr);
    u64 h[K_N];
    DEVCHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st)); // (the views' host images and hv were read by the copies above before this returns)
    DEVCHK(hipGetLastError());
    S[1] = (double)h[K_COLOURED];
    S[2] = (double)h[K_NONORMAL];
    S[3] = (double)h[K_VISIBLE];
    S[4] = (double)h[K_DRAWN];
    S[5] = (double)h[K_BIG];
    if (stats) memcpy(stats, S, sizeof S);
    scene->d_views = d_views;
    scene->V = V;
    scene->row = row;
    scene->corner = corner;
    return RSM_OK;
}

int mesh_color_device(const float *d_v, int64_t nv, const int32_t *d_f, int64_t nf, const rsm_dedup_view *views, int n_pairs, const rsm_mesh_color_params *p,
                      long long big_box, uint8_t *d_rgb, int32_t *d_best, double *stats, int *invalid, hipStream_t st) {
    DevMem M;
    McScene scene;
    return mesh_color_scene_device(M, d_v, nv, d_f, nf, views, n_pairs, p, big_box, d_rgb, d_best, nullptr, stats, invalid, &scene, st);
}
