// k_dedup.hip -- multi-view duplicate deletion of the merged cloud, the isdelete branch of CCloudOptimization::run
// (CloudOptimization/CCloudOptimization.cpp:152-346), SURVEY 8(f6).  Overlapping pairs of a rig each put a layer of points on the
// surfaces they share; the branch projects every merged point into the left view of the pair it faces best, buckets the points by
// pixel and keeps one point per surface layer per pixel.  Restated rule by rule (DESIGN 9 f6 lists the places the reference leaves
// undefined and how they are defined here; tests/dedup_restatement.py is the same in numpy):
//   assign (:160-192), per point j in index order: best pair b = first maximum of n.(C_i - p) / |C_i - p| (float, strict '<'
//     from FLT_MIN: pair 0 when nothing exceeds it); q = R[b][0] p + T[b][0]; x = ROUND(q0 / q2) - XL, y = ROUND(q1 / q2) - YL
//     (SharedInclude.h:48: float quotient, double + 0.5, truncation); outside the bound -> s1, left mask 0 -> s2, else j joins
//     bucket[b][y][x] (ascending j);
//   select (:205-337), pairs, rows, columns in order, pixels whose left mask is 255 only: size 1 -> emit; size 2 -> both when the
//     normals' dot is < 0, else the first k whose right projection lands on mask 255 if CurrentValue > -1; size >= 3 -> order by
//     |p - C| descending (stable), split into runs of equal direction n.(p - C) < 0, one point per run (the right-mask / NCC
//     rule for runs of two or more, the run's farthest when nothing passes), the nearest never emitted.
//   CurrentValue: the fp64 NCC of the 5x5x3 windows at the LEFT pixel (x - 2, y - 2) of both images (:254, :322: the right window
//     is not at the projection), cv::Mat WindowToVec gather (CManageData.h:45-59: row outer, byte inner), Armadillo's
//     two-accumulator mean / norm / dot.
// Kernels: k_dedup_assign writes one key per point (pair base + (y - YL) * width + (x - XL), or a sentinel after every bucket);
// rocprim's stable radix sort on only the key bits in use restores the push_back order inside each bucket; k_dedup_select runs
// one thread per bucket start and writes the bucket's emitted indices into its own slice of a scratch array plus a count; the
// counts' exclusive scan and k_dedup_write give indicesptr in (pair, y, x) order -- the reference's visiting order.
#include "../../include/rsm.h"
#include "cloud_arena.h"
#include "dev_prims.h"
#include "project_common.h"

#include <float.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int DD_R = 2;                     // MatchBlockRadius of the branch (:199), independent of the matcher's
constexpr int DD_W = 2 * DD_R + 1;          // window_size
constexpr int DD_N = DD_W * DD_W * 3;       // vec_size

// (dd_dot3, dd_round, dd_project: project_common.h, shared with k_meshcolor.hip)

__device__ __forceinline__ void wave_add(unsigned long long *ctr, bool v) {
    // one atomic per wave for a flag most lanes may raise (every lane of the wave calls it)
    const unsigned long long act = __ballot(1), set = __ballot(v);
    const int leader = __ffsll((long long)act) - 1;
    if ((int)__lane_id() == leader && set) atomicAdd(ctr, (unsigned long long)__popcll(set));
}

template <typename K>
__global__ __launch_bounds__(256) void k_dedup_assign(const float *__restrict__ pts, int stride, const float4 *__restrict__ nrm, int n,
                                                      const DedupPair *__restrict__ P, int np, K sentinel, K *__restrict__ keys,
                                                      uint32_t *__restrict__ vals, unsigned long long *__restrict__ ctr) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    int why = 0; // 1: s1, 2: s2
    if (j < n) {
        const float px = pts[(size_t)stride * j], py = pts[(size_t)stride * j + 1], pz = pts[(size_t)stride * j + 2];
        const float4 nv = nrm[j];
        float best = FLT_MIN;
        int b = 0;
        for (int i = 0; i < np; i++) {
            const float cx = P[i].C[0] - px, cy = P[i].C[1] - py, cz = P[i].C[2] - pz;
            const float v = dd_dot3(nv.x, nv.y, nv.z, cx, cy, cz) / sqrtf(dd_dot3(cx, cy, cz, cx, cy, cz));
            if (best < v) {
                best = v;
                b = i;
            }
        }
        const DedupPair &c = P[b];
        long long x, y;
        K key = sentinel;
        if (!dd_project(c.R0, c.T0, px, py, pz, &x, &y)) why = 1;
        else {
            x -= c.XL;
            y -= c.YL;
            if (x < 0 || x >= c.bw || y < 0 || y >= c.bh) why = 1; // (an empty bound: bw or bh <= 0)
            else if (c.m0[(size_t)(y + c.YL) * c.W + (size_t)(x + c.XL)] == 0) why = 2;
            else key = (K)(c.base + (unsigned long long)(y * c.bw + x));
        }
        keys[j] = key;
        vals[j] = (uint32_t)j;
    }
    wave_add(&ctr[0], why == 1);
    wave_add(&ctr[1], why == 2);
}

// CurrentValue of pixel (X, Y) of pair c: arma::dot(vecL, vecR) / (normR * normL), windows at (X - 2, Y - 2) of both images
__device__ double dd_ncc(const DedupPair &c, int X, int Y) {
    const size_t row = (size_t)c.W * 3;
    const uint8_t *a = c.img0 + (size_t)(Y - DD_R) * row + (size_t)(X - DD_R) * 3;
    const uint8_t *b = c.img1 + (size_t)(Y - DD_R) * row + (size_t)(X - DD_R) * 3;
    int sa = 0, sb = 0;
    for (int i = 0; i < DD_W; i++)
        for (int k = 0; k < 3 * DD_W; k++) {
            sa += a[i * row + k];
            sb += b[i * row + k];
        }
    const double ma = (double)sa / (double)DD_N, mb = (double)sb / (double)DD_N; // accumulate / n: the byte sums are exact
    double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0, d1 = 0.0, d2 = 0.0;
    int t = 0; // the vector's element index: k = row * 15 + byte
    for (int i = 0; i < DD_W; i++)
        for (int k = 0; k < 3 * DD_W; k++, t++) {
            const double u = (double)a[i * row + k] - ma, v = (double)b[i * row + k] - mb;
            if (t & 1) {
                a2 += u * u;
                b2 += v * v;
                d2 += u * v;
            } else {
                a1 += u * u;
                b1 += v * v;
                d1 += u * v;
            }
        }
    double nl = sqrt(a1 + a2), nr = sqrt(b1 + b2);
    if (nl == 0) nl = 1;
    if (nr == 0) nr = 1;
    return (d1 + d2) / (nr * nl);
}

// the right view's test of :246-253: projection with R[i][1], T[i][1] (no bound subtracted) onto right-mask 255
__device__ __forceinline__ bool dd_right_ok(const DedupPair &c, const float *pts, int stride, uint32_t idx) {
    long long x, y;
    if (!dd_project(c.R1, c.T1, pts[(size_t)stride * idx], pts[(size_t)stride * idx + 1], pts[(size_t)stride * idx + 2], &x, &y)) return false;
    if (x < 0 || x >= c.W || y < 0 || y >= c.H) return false;
    return c.m1[(size_t)y * c.W + (size_t)x] == 255;
}

// one thread per sorted position; bucket starts run the selection.  Emitted indices go to tmp[j ..), their count to cnt[j];
// buckets of three or more order their members through dsc / osc[j ..) (the bucket's own slice: no size cap)
template <typename K>
__global__ __launch_bounds__(256) void k_dedup_select(const K *__restrict__ keys, const uint32_t *__restrict__ vals, int nv,
                                                      const float *__restrict__ pts, int stride, const float4 *__restrict__ nrm,
                                                      const DedupPair *__restrict__ P, int np, uint32_t *__restrict__ cnt,
                                                      int32_t *__restrict__ tmp, float *__restrict__ dsc, uint32_t *__restrict__ osc,
                                                      unsigned long long *__restrict__ ctr) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    bool visit = false;
    unsigned long long miss = 0;
    if (j < nv) {
        const K key = keys[j];
        int emitted = 0;
        if (j == 0 || keys[j - 1] != key) {
            int e = j + 1;
            while (e < nv && keys[e] == key) e++;
            const int sz = e - j;
            int i = 0; // the non-empty pair whose key range holds the bucket
            for (int t = 0; t < np; t++)
                if (P[t].bw > 0 && P[t].bh > 0 && P[t].base <= (unsigned long long)key) i = t;
            const DedupPair &c = P[i];
            const long long rel = (long long)((unsigned long long)key - c.base);
            const int X = (int)(rel % c.bw) + c.XL, Y = (int)(rel / c.bw) + c.YL;
            if (c.m0[(size_t)Y * c.W + X] == 255) { // :216
                visit = true;
                bool have_cv = false;
                double cv = 0.0;
                if (sz == 1) {
                    tmp[j] = (int32_t)vals[j];
                    emitted = 1;
                } else if (sz == 2) {
                    const uint32_t a = vals[j], b = vals[j + 1];
                    const float4 na = nrm[a], nb = nrm[b];
                    if (dd_dot3(na.x, na.y, na.z, nb.x, nb.y, nb.z) < 0) { // :231-237
                        tmp[j] = (int32_t)a;
                        tmp[j + 1] = (int32_t)b;
                        emitted = 2;
                    } else {
                        int win = -1;
                        double bestv = -1.0;
                        for (int k = 0; k < 2; k++) {
                            if (!dd_right_ok(c, pts, stride, vals[j + k])) {
                                miss++;
                                continue;
                            }
                            if (!have_cv) {
                                cv = dd_ncc(c, X, Y);
                                have_cv = true;
                            }
                            if (cv > bestv) {
                                win = k;
                                bestv = cv;
                            }
                        }
                        if (win >= 0) {
                            tmp[j] = (int32_t)vals[j + win];
                            emitted = 1;
                        }
                    }
                } else {
                    // distances and directions (:276-281); d not > 0 (0 or NaN) sorts after every other, in bucket order
                    int nvalid = 0;
                    for (int l = 0; l < sz; l++) {
                        const uint32_t q = vals[j + l];
                        const float dx = pts[(size_t)stride * q] - c.C[0], dy = pts[(size_t)stride * q + 1] - c.C[1],
                                    dz = pts[(size_t)stride * q + 2] - c.C[2];
                        const float d = sqrtf(dd_dot3(dx, dy, dz, dx, dy, dz));
                        dsc[j + l] = d;
                        nvalid += d > 0.0f;
                    }
                    // the repeated first-maximum selection (:282-296) = a stable sort by distance, descending: rank by counting
                    for (int l = 0; l < sz; l++) {
                        const float d = dsc[j + l];
                        int r = 0;
                        if (d > 0.0f) {
                            for (int m = 0; m < sz; m++) {
                                const float o = dsc[j + m];
                                r += (o > d) || (m < l && o == d);
                            }
                        } else {
                            r = nvalid;
                            for (int m = 0; m < l; m++) r += !(dsc[j + m] > 0.0f);
                        }
                        const uint32_t q = vals[j + l];
                        const float4 nq = nrm[q];
                        const float dx = pts[(size_t)stride * q] - c.C[0], dy = pts[(size_t)stride * q + 1] - c.C[1],
                                    dz = pts[(size_t)stride * q + 2] - c.C[2];
                        const uint32_t dir = dd_dot3(nq.x, nq.y, nq.z, dx, dy, dz) < 0;
                        osc[j + r] = (uint32_t)l | (dir << 31);
                    }
                    // runs of equal direction (:298-334)
                    int last = 0;
                    for (int l = 1; l < sz; l++) {
                        if ((osc[j + last] >> 31) == (osc[j + l] >> 31) && l != sz - 1) continue;
                        int ti = last;
                        if (last + 1 < l) {
                            double bestv = -1.0;
                            for (int k = last; k < l; k++) {
                                if (!dd_right_ok(c, pts, stride, vals[j + (osc[j + k] & 0x7fffffffu)])) {
                                    miss++;
                                    continue;
                                }
                                if (!have_cv) {
                                    cv = dd_ncc(c, X, Y);
                                    have_cv = true;
                                }
                                if (cv > bestv) {
                                    ti = k;
                                    bestv = cv;
                                }
                            }
                        }
                        tmp[j + emitted++] = (int32_t)vals[j + (osc[j + ti] & 0x7fffffffu)];
                        last = l;
                    }
                }
            }
        }
        cnt[j] = (uint32_t)emitted;
    }
    if (miss) atomicAdd(&ctr[2], miss);
    wave_add(&ctr[3], visit);
}

__global__ void k_dedup_write(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off, const int32_t *__restrict__ tmp, int nv,
                              int32_t *__restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nv) return;
    const uint32_t c = cnt[j], o = off[j];
    for (uint32_t t = 0; t < c; t++) out[o + t] = tmp[j + t];
}

__global__ void k_dedup_gather(const float4 *__restrict__ rec, const float4 *__restrict__ nrm, const int32_t *__restrict__ idx, int m,
                               float4 *__restrict__ orec, float4 *__restrict__ onrm) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int32_t i = idx[k];
    if (orec) orec[k] = rec[i];
    if (onrm) onrm[k] = nrm[i];
}

template <typename K>
size_t sort_scan_bytes(int64_t n) {
    size_t sb = 0, cb = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sb, (K *)nullptr, (K *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n, 0, 8 * sizeof(K));
    (void)rocprim::exclusive_scan(nullptr, cb, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>());
    return sb + cb;
}

template <typename K>
int dedup_run(FilterArena *A, const float *d_pts, int stride, const float4 *d_nrm, int n, const DedupPair *d_pairs, int np, unsigned long long total, int32_t *d_index, int64_t *n_out, int64_t stats[4], hipStream_t st) {
    unsigned long long *ctr = A->get<unsigned long long>(4);
    K *k0 = A->get<K>((size_t)n), *k1 = A->get<K>((size_t)n);
    uint32_t *v0 = A->get<uint32_t>((size_t)n), *v1 = A->get<uint32_t>((size_t)n);
    unsigned long long *h = (unsigned long long *)filter_arena_host(A); // [0..3] counters, [4] the last offset and count
    if (!ctr || !k0 || !k1 || !v0 || !v1 || !h) return RSM_E_NOMEM;
    DEVCHK(hipMemsetAsync(ctr, 0, 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_dedup_assign<K>, blocks_for(n), dim3(256), 0, st, d_pts, stride, d_nrm, n, d_pairs, np, (K)total, k0, v0, ctr);
    // keys 0 .. total (the sentinel): only the bits in use
    int s = sort_pairs(*A, k0, k1, v0, v1, (size_t)n, key_bits(total), st);
    if (s != RSM_OK) return s;
    DEVCHK(hipMemcpyAsync(h, ctr, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    DEVCHK(hipStreamSynchronize(st));
    const int nv = n - (int)(h[0] + h[1]);
    stats[0] = (int64_t)h[0];
    stats[1] = (int64_t)h[1];
    if (nv > 0) {
        uint32_t *cnt = A->get<uint32_t>((size_t)nv), *off = A->get<uint32_t>((size_t)nv);
        int32_t *tmp = A->get<int32_t>((size_t)nv);
        float *dsc = A->get<float>((size_t)nv);
        uint32_t *osc = A->get<uint32_t>((size_t)nv);
        if (!cnt || !off || !tmp || !dsc || !osc) return RSM_E_NOMEM;
        const dim3 gv = blocks_for(nv);
        hipLaunchKernelGGL(k_dedup_select<K>, gv, dim3(256), 0, st, k1, v1, nv, d_pts, stride, d_nrm, d_pairs, np, cnt, tmp, dsc, osc, ctr);
        if ((s = scan_u32(*A, cnt, off, (size_t)nv, st)) != RSM_OK) return s;
        hipLaunchKernelGGL(k_dedup_write, gv, dim3(256), 0, st, cnt, off, tmp, nv, d_index);
        uint64_t emitted = 0;
        DEVCHK(hipMemcpyAsync(&h[2], &ctr[2], 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st)); // (read back with the total)
        if ((s = scan_total(cnt, off, (size_t)nv, st, &emitted, (unsigned int *)(h + 4))) != RSM_OK) return s;
        stats[2] = (int64_t)h[2];
        stats[3] = (int64_t)h[3];
        *n_out = (int64_t)emitted;
    } else {
        stats[2] = stats[3] = 0;
        *n_out = 0;
    }
    return hipGetLastError() == hipSuccess ? RSM_OK : RSM_E_HIP;
}

bool bound_empty(const rsm_boundary &b) { return b.width <= 0 || b.height <= 0; }

} // namespace

int dedup_views_ok(const rsm_dedup_view *v, int np) {
    for (int i = 0; i < np; i++) {
        const rsm_dedup_view &w = v[i];
        if (w.width < 2 * DD_R + 1 || w.height < 2 * DD_R + 1 || !w.image[0] || !w.image[1] || !w.mask[0] || !w.mask[1]) return 0;
        const rsm_boundary &b = w.bound0;
        if (bound_empty(b)) continue; // owns no buckets: its points count in s1
        if (b.width != b.XR - b.XL + 1 || b.height != b.YR - b.YL + 1) return 0;
        // the 5 x 5 windows of every bucket pixel must lie inside the image
        if (b.XL < DD_R || b.YL < DD_R || b.XR > w.width - 1 - DD_R || b.YR > w.height - 1 - DD_R) return 0;
    }
    return 1;
}

static unsigned long long dedup_total_keys(const rsm_dedup_view *v, int np) {
    unsigned long long t = 0;
    for (int i = 0; i < np; i++)
        if (!bound_empty(v[i].bound0)) t += (unsigned long long)v[i].bound0.width * (unsigned long long)v[i].bound0.height;
    return t;
}

size_t dedup_arena_bytes(const rsm_dedup_view *v, int np, int64_t n) {
    size_t img = 0;
    for (int i = 0; i < np; i++) img += ((size_t)v[i].width * v[i].height * 3 + 256) * 2 + ((size_t)v[i].width * v[i].height + 256) * 2;
    const bool k64 = dedup_total_keys(v, np) >= 0xffffffffull;
    const size_t per = k64 ? 2 * 8 + 8 + 20 : 2 * 4 + 8 + 20; // keys x2, values x2, counts / offsets / emitted / distances / order
    return img + (size_t)np * sizeof(DedupPair) + 4096 + (size_t)n * per + (k64 ? sort_scan_bytes<unsigned long long>(n) : sort_scan_bytes<uint32_t>(n)) +
           (size_t)16 * 256;
}

int dedup_cloud_device(FilterArena *A, const float *d_pts, int stride, const float4 *d_nrm, int64_t n, const rsm_dedup_view *v, int np,
                       int32_t *d_index, int64_t *n_out, int64_t stats[4], hipStream_t st) {
    *n_out = 0;
    for (int t = 0; t < 4; t++) stats[t] = 0;
    if (n <= 0) return RSM_OK;
    if (n > (int64_t)INT32_MAX || np < 1 || !dedup_views_ok(v, np)) return RSM_E_INVALID;
    // the pairs' images and masks on the device, R / T as float (cv2eigen of P's columns, CCloudOptimization.cpp:68-71)
    std::vector<DedupPair> hp((size_t)np);
    unsigned long long base = 0;
    for (int i = 0; i < np; i++) {
        const rsm_dedup_view &w = v[i];
        DedupPair &c = hp[(size_t)i];
        memset(&c, 0, sizeof(c));
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) {
                c.R0[3 * r + k] = (float)w.P[0][4 * r + k];
                c.R1[3 * r + k] = (float)w.P[1][4 * r + k];
            }
            c.T0[r] = (float)w.P[0][4 * r + 3];
            c.T1[r] = (float)w.P[1][4 * r + 3];
            c.C[r] = w.cam_center[r];
        }
        c.XL = w.bound0.XL;
        c.YL = w.bound0.YL;
        c.bw = w.bound0.width;
        c.bh = w.bound0.height;
        c.W = w.width;
        c.H = w.height;
        c.base = base;
        if (!bound_empty(w.bound0)) base += (unsigned long long)c.bw * (unsigned long long)c.bh;
        const size_t pix = (size_t)w.width * w.height;
        uint8_t *d[4];
        for (int k = 0; k < 4; k++) {
            d[k] = A->get<uint8_t>(k < 2 ? 3 * pix : pix);
            if (!d[k]) return RSM_E_NOMEM;
            const uint8_t *src = k < 2 ? w.image[k] : w.mask[k - 2];
            if (hipMemcpyAsync(d[k], src, k < 2 ? 3 * pix : pix, hipMemcpyHostToDevice, st) != hipSuccess) return RSM_E_HIP;
        }
        c.img0 = d[0];
        c.img1 = d[1];
        c.m0 = d[2];
        c.m1 = d[3];
    }
    if (base == 0) { // no pair owns a bucket: every point is outside
        stats[0] = n;
        return RSM_OK;
    }
    DedupPair *dp = A->get<DedupPair>((size_t)np);
    if (!dp) return RSM_E_NOMEM;
    if (hipMemcpyAsync(dp, hp.data(), sizeof(DedupPair) * (size_t)np, hipMemcpyHostToDevice, st) != hipSuccess) return RSM_E_HIP;
    // (the staged host vector is read by the copy before the first synchronisation inside dedup_run)
    if (base < 0xffffffffull)
        return dedup_run<uint32_t>(A, d_pts, stride, d_nrm, (int)n, dp, np, base, d_index, n_out, stats, st);
    return dedup_run<unsigned long long>(A, d_pts, stride, d_nrm, (int)n, dp, np, base, d_index, n_out, stats, st);
}

void launch_dedup_gather(const void *d_rec, const float *d_nrm, const int32_t *d_idx, int64_t m, void *d_orec, float *d_onrm, hipStream_t st) {
    if (m > 0)
        hipLaunchKernelGGL(k_dedup_gather, blocks_for(m), dim3(256), 0, st, (const float4 *)d_rec, (const float4 *)d_nrm, d_idx,
                           (int)m, (float4 *)d_orec, (float4 *)d_onrm);
}
