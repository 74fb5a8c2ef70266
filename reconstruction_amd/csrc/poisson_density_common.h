// poisson_density_common.h -- what the units that splat a sample at the two levels around its depth share (k_poisson_density.hip,
// k_poisson_band_density.hip): the coarsest level, and how a depth splits.
#pragma once

#include <math.h>

#define PD_LMIN 3           // the coarsest level a sample is spread on

// d_s on a grid whose finest level is `depth`: *lo = floor(d_s) in PD_LMIN..depth, returns fr = d_s - lo.  (k_pd_sample clamped d_s to
// PD_LMIN..the call's depth; a coarser problem on the same samples clamps again here, and the level stays inside the buffer whatever d holds)
__device__ __forceinline__ double pd_split(double ds, int depth, int *lo) {
    ds = ds < (double)depth ? ds : (double)depth;
    const double fld = floor(ds);
    int l = ds >= (double)PD_LMIN ? (int)fld : PD_LMIN;
    *lo = l > depth ? depth : l;
    return ds - fld;
}
// the share of w_s at level lo (t = 0) and at lo + 1 (t = 1)
__device__ __forceinline__ double pd_alpha(double fr, double ws, int t) { return t ? fr * ws : (1.0 - fr) * ws; }
