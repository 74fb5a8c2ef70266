// k_mls.hip -- moving-least-squares smoothing of the merged cloud, CCloudOptimization::run (CloudOptimization/
// CCloudOptimization.cpp:348-389), SURVEY 8(f5): pcl::MovingLeastSquaresOMP with setComputeNormals(true), setSearchRadius(
// m_mls_radius), setPolynomialFit(true), setPolynomialOrder(1), no upsampling, then the output normals turned to agree with the
// filter's normals of the same input points (:378-385).
// PCL is not in the reference tree; MovingLeastSquares::computeMLSPointNormal (upsampling NONE) is restated from PCL 1.7.2's
// published sources as oracle/cloud_oracle.c restates the filter (parity unpinned), per input point p:
//   neighbours: the finite q with float32 (dx^2 + dy^2) + dz^2 < r^2, p included; fewer than 3: no output;
//   plane: double centroid c, de-meaned covariance sum (q - c)(q - c)^T (two passes: compute3DCentroid + computeCovarianceMatrix),
//     eigen33 (pcl_plane_from_cov): unit normal n of the smallest eigenvalue, curvature |lambda / trace|; pt = p - (n.p - n.c) n;
//   polynomial (order > 0 and at least (order + 1)(order + 2) / 2 neighbours): v = n.unitOrthogonal() (Eigen's rule), u = n x v;
//     per neighbour e = q - pt, w = exp(-(e.e) / r^2), terms uc^i vc^j in PCL's order; (P W P^T) c = P W f by Cholesky in double;
//     c[0] finite: pt += c[0] n, normal = n - (c[order + 1] u + c[1] v) -- NOT renormalised, as PCL 1.7.2 leaves it.
//     A Cholesky pivot that is not positive (Eigen's LLT reports failure and its solve is then undefined) counts as no fit.
// Outputs in input order (the serial form of the OMP loop; its thread chunks are not deterministic) with their input index.
//
// Kernel: one thread per point of the radius-cell grid's sorted order (cell edge r: the 27 cells around p cover the ball),
// walking the 9 key ranges three times -- count + centroid, covariance, the weighted normal equations (9 doubles for order 1,
// 27 for order 2, a double exp per neighbour).  Results land at the input index with a flag; the flags' exclusive scan and a
// compaction give the input order (as the filter's k_keep_flags / k_compact_kept).
#include "../../include/rsm.h"
#include "cloud_grid.h"

#include <algorithm>
#include <cmath>

__global__ void k_point16_xyz(const float4 *__restrict__ rec, int64_t n, float *__restrict__ xyz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 r = rec[i]; // {x, y, z, bgr + pad}
    xyz[3 * i] = r.x;
    xyz[3 * i + 1] = r.y;
    xyz[3 * i + 2] = r.z;
}

template <int ORDER>
__global__ __launch_bounds__(256) void k_mls(const float4 *__restrict__ sxyz, const unsigned long long *__restrict__ keys, int nv, FGrid g, float r2,
                                             double gauss, const float4 *__restrict__ ref, float *__restrict__ txyz, float4 *__restrict__ tnrm,
                                             unsigned int *__restrict__ flag) {
    constexpr int NC = (ORDER + 1) * (ORDER + 2) / 2; // nr_coeff_
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nv) return;
    const float4 p = sxyz[j];
    const unsigned int i = __float_as_uint(p.w);
    int rs[9], re[9];
    ranges9(keys, nv, g, p.x, p.y, p.z, rs, re);
    // pass 1: neighbours and their centroid (compute3DCentroid)
    int cnt = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int r = 0; r < 9; r++)
        for (int q = rs[r]; q < re[r]; q++) {
            const float4 o = sxyz[q];
            if (!(fdist2(p.x, p.y, p.z, o.x, o.y, o.z) < r2)) continue;
            sx += (double)o.x; sy += (double)o.y; sz += (double)o.z;
            cnt++;
        }
    if (cnt < 3) return; // (flag stays 0)
    const double cx = sx / (double)cnt, cy = sy / (double)cnt, cz = sz / (double)cnt;
    // pass 2: the de-meaned covariance (computeCovarianceMatrix, not normalised)
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
#pragma unroll
    for (int r = 0; r < 9; r++)
        for (int q = rs[r]; q < re[r]; q++) {
            const float4 o = sxyz[q];
            if (!(fdist2(p.x, p.y, p.z, o.x, o.y, o.z) < r2)) continue;
            const double dx = (double)o.x - cx, dy = (double)o.y - cy, dz = (double)o.z - cz;
            c00 += dx * dx; c01 += dx * dy; c02 += dx * dz;
            c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
        }
    double cov[9] = {c00, c01, c02, c01, c11, c12, c02, c12, c22};
    double n[3], curv;
    pcl_plane_from_cov(cov, n, &curv);
    const double d = -((n[0] * cx + n[1] * cy) + n[2] * cz);
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    const double dist = ((px * n[0] + py * n[1]) + pz * n[2]) + d;
    double tx = px - dist * n[0], ty = py - dist * n[1], tz = pz - dist * n[2];
    double nx = n[0], ny = n[1], nz = n[2];
    if constexpr (ORDER > 0) if (cnt >= NC) {
        // Darboux frame: v = n.unitOrthogonal() (Eigen: unitOrthogonal_selector<.., 3>, isMuchSmallerThan with precision 1e-12)
        double v[3];
        if (fabs(n[0]) > fabs(n[2]) * 1e-12 || fabs(n[1]) > fabs(n[2]) * 1e-12) {
            const double inv = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1]);
            v[0] = -n[1] * inv; v[1] = n[0] * inv; v[2] = 0.0;
        } else {
            const double inv = 1.0 / sqrt(n[1] * n[1] + n[2] * n[2]);
            v[0] = 0.0; v[1] = -n[2] * inv; v[2] = n[1] * inv;
        }
        const double u[3] = {n[1] * v[2] - n[2] * v[1], n[2] * v[0] - n[0] * v[2], n[0] * v[1] - n[1] * v[0]};
        // pass 3: the normal equations, upper triangle of P W P^T (row-major) and P W f
        double A[NC * (NC + 1) / 2], b[NC];
#pragma unroll
        for (int k = 0; k < NC * (NC + 1) / 2; k++) A[k] = 0.0;
#pragma unroll
        for (int k = 0; k < NC; k++) b[k] = 0.0;
#pragma unroll
        for (int r = 0; r < 9; r++)
            for (int q = rs[r]; q < re[r]; q++) {
                const float4 o = sxyz[q];
                if (!(fdist2(p.x, p.y, p.z, o.x, o.y, o.z) < r2)) continue;
                const double ex = (double)o.x - tx, ey = (double)o.y - ty, ez = (double)o.z - tz;
                const double w = exp(-((ex * ex + ey * ey) + ez * ez) / gauss);
                const double uc = (ex * u[0] + ey * u[1]) + ez * u[2];
                const double vc = (ex * v[0] + ey * v[1]) + ez * v[2];
                const double f = (ex * n[0] + ey * n[1]) + ez * n[2];
                double P[NC];
                int t = 0;
                double u_pow = 1.0;
#pragma unroll
                for (int ui = 0; ui <= ORDER; ui++) {
                    double v_pow = 1.0;
#pragma unroll
                    for (int vi = 0; vi <= ORDER - ui; vi++) {
                        P[t++] = u_pow * v_pow;
                        v_pow *= vc;
                    }
                    u_pow *= uc;
                }
                int a = 0;
#pragma unroll
                for (int k = 0; k < NC; k++) {
                    const double pw = P[k] * w;
#pragma unroll
                    for (int l = k; l < NC; l++) A[a++] += pw * P[l];
                    b[k] += pw * f;
                }
            }
        // LLT in registers: A = L L^T (L overwrites the lower triangle of a full copy), then L y = b, L^T c = y
        double L[NC][NC];
        {
            int a = 0;
#pragma unroll
            for (int k = 0; k < NC; k++)
#pragma unroll
                for (int l = k; l < NC; l++) {
                    L[k][l] = A[a];
                    L[l][k] = A[a++];
                }
        }
        bool ok = true;
#pragma unroll
        for (int k = 0; k < NC; k++) {
            double x = L[k][k];
#pragma unroll
            for (int m = 0; m < k; m++) x -= L[k][m] * L[k][m];
            ok = ok && x > 0.0;
            const double dkk = sqrt(x);
            L[k][k] = dkk;
#pragma unroll
            for (int r = k + 1; r < NC; r++) {
                double s = L[r][k];
#pragma unroll
                for (int m = 0; m < k; m++) s -= L[r][m] * L[k][m];
                L[r][k] = s / dkk;
            }
        }
        double c[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) {
            double s = b[k];
#pragma unroll
            for (int m = 0; m < k; m++) s -= L[k][m] * c[m];
            c[k] = s / L[k][k];
        }
#pragma unroll
        for (int k = NC - 1; k >= 0; k--) {
            double s = c[k];
#pragma unroll
            for (int m = k + 1; m < NC; m++) s -= L[m][k] * c[m];
            c[k] = s / L[k][k];
        }
        if (ok && isfinite(c[0])) {
            tx += c[0] * n[0]; ty += c[0] * n[1]; tz += c[0] * n[2];
            nx = n[0] - (c[ORDER + 1] * u[0] + c[1] * v[0]);
            ny = n[1] - (c[ORDER + 1] * u[1] + c[1] * v[1]);
            nz = n[2] - (c[ORDER + 1] * u[2] + c[1] * v[2]);
        }
    }
    float fx = (float)nx, fy = (float)ny, fz = (float)nz;
    if (ref) { // :378-385: flip to agree with the input point's filter normal (a NaN one never flips)
        const float4 rn = ref[i];
        if ((fx * rn.x + fy * rn.y) + fz * rn.z < 0.0f) { fx = -fx; fy = -fy; fz = -fz; }
    }
    txyz[3 * (size_t)i] = (float)tx;
    txyz[3 * (size_t)i + 1] = (float)ty;
    txyz[3 * (size_t)i + 2] = (float)tz;
    tnrm[i] = make_float4(fx, fy, fz, (float)curv);
    flag[i] = 1u;
}

__global__ void k_mls_compact(const unsigned int *__restrict__ flag, const unsigned int *__restrict__ pos, int64_t n, const float *__restrict__ txyz,
                              const float4 *__restrict__ tnrm, float *__restrict__ oxyz, float *__restrict__ onrm, int32_t *__restrict__ oidx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const size_t o = pos[i];
    oxyz[3 * o] = txyz[3 * i];
    oxyz[3 * o + 1] = txyz[3 * i + 1];
    oxyz[3 * o + 2] = txyz[3 * i + 2];
    const float4 v = tnrm[i];
    onrm[4 * o] = v.x;
    onrm[4 * o + 1] = v.y;
    onrm[4 * o + 2] = v.z;
    onrm[4 * o + 3] = v.w;
    oidx[o] = (int32_t)i;
}

void launch_point16_xyz(const void *rec, int64_t n, float *xyz, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_point16_xyz, blocks_for(n), dim3(256), 0, st, (const float4 *)rec, n, xyz);
}

size_t mls_arena_bytes(int64_t n) { // grid (keys x2, values x2, sorted points), staged results, flags + positions, sort / scan temporaries
    size_t sort_bytes = 0, scan_bytes = 0; // (what build_grid's radix sort and the compaction's scan ask for at this size)
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, (unsigned int *)nullptr,
                                    (unsigned int *)nullptr, (size_t)n, 0, 64);
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, (unsigned int *)nullptr, (unsigned int *)nullptr, 0u, (size_t)n, rocprim::plus<unsigned int>());
    return (size_t)n * (16 + 8 + 16 + 12 + 16 + 8) + sort_bytes + scan_bytes + (size_t)64 * 256;
}

int mls_cloud_device(FilterArena *A, const float *d_xyz, int64_t n, const float4 *d_ref, double radius, int order, float *d_oxyz, float *d_onrm,
                     int32_t *d_oidx, int64_t *n_out, hipStream_t st) {
    *n_out = 0;
    if (n <= 0) return RSM_OK;
    if (n > (int64_t)INT32_MAX || !(radius > 0.0) || order < 0 || order > 2) return RSM_E_INVALID;
    float lo[3], hi[3];
    int64_t nv = 0;
    int s = cloud_bbox(A, d_xyz, n, st, lo, hi, &nv);
    if (s != RSM_OK) return s;
    if (nv == 0) return RSM_OK;
    float *txyz = A->get<float>(3 * (size_t)n);
    float4 *tnrm = A->get<float4>((size_t)n);
    unsigned int *flag = A->get<unsigned int>((size_t)n), *pos = A->get<unsigned int>((size_t)n);
    if (!txyz || !tnrm || !flag || !pos) return RSM_E_NOMEM;
    FilterGridDev G;
    s = build_grid(A, d_xyz, n, 0 /* no table: ranges by binary search, as the filter's normals */, (float)radius, lo, hi, st, G);
    if (s != RSM_OK) return s;
    DEVCHK(hipMemsetAsync(flag, 0, sizeof(unsigned int) * (size_t)n, st));
    const float r2 = (float)(radius * radius);
    const double gauss = radius * radius; // sqr_gauss_param_ (setSearchRadius sets it to radius^2)
    const dim3 grid = blocks_for(nv);
    if (order == 0)
        hipLaunchKernelGGL(k_mls<0>, grid, dim3(256), 0, st, G.sxyz, G.keys, (int)nv, G.g, r2, gauss, d_ref, txyz, tnrm, flag);
    else if (order == 1)
        hipLaunchKernelGGL(k_mls<1>, grid, dim3(256), 0, st, G.sxyz, G.keys, (int)nv, G.g, r2, gauss, d_ref, txyz, tnrm, flag);
    else
        hipLaunchKernelGGL(k_mls<2>, grid, dim3(256), 0, st, G.sxyz, G.keys, (int)nv, G.g, r2, gauss, d_ref, txyz, tnrm, flag);
    if ((s = scan_u32(*A, flag, pos, (size_t)n, st)) != RSM_OK) return s;
    hipLaunchKernelGGL(k_mls_compact, blocks_for(n), dim3(256), 0, st, flag, pos, n, txyz, tnrm, d_oxyz, d_onrm, d_oidx);
    uint64_t total = 0;
    if ((s = scan_total(flag, pos, (size_t)n, st, &total, (unsigned int *)filter_arena_host(A))) != RSM_OK) return s;
    DEVCHK(hipGetLastError());
    *n_out = (int64_t)total;
    return RSM_OK;
}
