// project_common.h -- the reference's projection of a point into a rectified view, shared by the duplicate deletion (k_dedup.hip) and the
// mesh colouring (k_meshcolor.hip): Eigen's 3-vector reductions in one order, ROUND of SharedInclude.h:48, and R p + T -> pixel.
#pragma once

#include <hip/hip_runtime.h>

// The Eigen 3-vector reductions (dot, squared norm, the rows of R p) all go through this one helper: (a0 b0 + a1 b1) + a2 b2, the
// order k_mls's flip and tests/mls_restatement.py use.  Whether Eigen 3's unrolled redux gives a0 b0 + (a1 b1 + a2 b2) instead is
// open; tests/dedup_restatement.py:_dot3 must change with it.
__device__ __forceinline__ float dd_dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// ROUND(x) = (int)((x) + 0.5) on a float quotient; false where the reference is undefined (non-finite, outside int)
__device__ __forceinline__ bool dd_round(float q, long long *r) {
    const double v = (double)q + 0.5;
    if (!(v > -2147483649.0 && v < 2147483648.0)) return false;
    *r = (long long)(int)v;
    return true;
}

__device__ __forceinline__ bool dd_project(const float *R, const float *T, float px, float py, float pz, long long *x, long long *y) {
    const float q0 = dd_dot3(R[0], R[1], R[2], px, py, pz) + T[0];
    const float q1 = dd_dot3(R[3], R[4], R[5], px, py, pz) + T[1];
    const float q2 = dd_dot3(R[6], R[7], R[8], px, py, pz) + T[2];
    return dd_round(q0 / q2, x) && dd_round(q1 / q2, y);
}
