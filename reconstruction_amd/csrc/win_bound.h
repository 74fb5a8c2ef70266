// win_bound.h -- the bound that makes the pixel lattice a search structure (k_filter_win.hip's head comment derives it): a point P of a depth map
// is farther than LB(w) from every ray at a pixel distance >= w + 1 from its own,
//     LB(w) = |F2| (w + 1) / (|P - T| |qz| / |F2| + w + 1),
// so a window of radius w holds every point closer than that.  The k-nearest passes (k_filter_win.hip) ask whether a given window decides a
// query (win_bound), the normals (k_filter.hip: k_normals_lattice) which window a given radius needs (win_need): one arithmetic, one set of margins.
#pragma once

#define WIN_PAD 40  // invalid-pixel border of the lattice copy (>= the largest window radius): no bounds checks in the loops
struct WinGeom {
    int gw, gh;         // lattice copy incl. the border: (XR - XL + 1 + 2 PAD) x (YR - YL + 1 + 2 PAD)
    double qz;          // Q[2][3] scaled (.cpp:698)
    double rz[3], T[3]; // third column of R_final (F2 = rz . (P - T)), T_final
};

// The rounding margins: a distance d counts as below the bound when d < LB (1 - WIN_M_LB) - WIN_M_COORD coord (float32 coordinates and
// float32 distance arithmetic: relative 1e-7 each), a squared one when d2 < lim^2 (1 - WIN_M_SQ); a search radius r is covered when even
// r (1 + WIN_M_R) is (its float32 square r2 and the squared test's margin).
constexpr double WIN_M_LB = 1e-5, WIN_M_COORD = 4e-7, WIN_M_SQ = 1e-6, WIN_M_R = 2e-6;

// the bound of a window of radius WR around P and its rounding margin, in double (once per query): the (k+1)-th smallest distance must stay
// below lim, its square tau below range (0: no positive bound)
struct WinBound {
    double lim;
    float range;
};
__device__ __forceinline__ WinBound win_bound(const float4 P, const WinGeom &g, int WR) {
    const double dx = (double)P.x - g.T[0], dy = (double)P.y - g.T[1], dz = (double)P.z - g.T[2];
    const double F2 = fabs(g.rz[0] * dx + g.rz[1] * dy + g.rz[2] * dz), nP = sqrt(dx * dx + dy * dy + dz * dz);
    const double iw = F2 / fabs(g.qz);                                   // |iW|: the lateral spacing of adjacent pixels at this depth
    const double LB = F2 * (WR + 1) / (nP / fmax(iw, 1e-300) + (WR + 1));
    const double coord = fmax(fmax(fabs((double)P.x), fabs((double)P.y)), fabs((double)P.z)) + nP;
    WinBound b;
    b.lim = LB * (1.0 - WIN_M_LB) - WIN_M_COORD * coord;
    b.range = (b.lim > 0.0) ? (float)(b.lim * b.lim * (1.0 - WIN_M_SQ)) : 0.0f;
    return b;
}
// ... inverted: the smallest w whose bound covers a radius search of r around P (1 << 20: none does)
__device__ __forceinline__ int win_need(const float4 P, const WinGeom &g, double r) {
    const double dx = (double)P.x - g.T[0], dy = (double)P.y - g.T[1], dz = (double)P.z - g.T[2];
    const double F2 = fabs(g.rz[0] * dx + g.rz[1] * dy + g.rz[2] * dz), nP = sqrt(dx * dx + dy * dy + dz * dz);
    const double iw = F2 / fabs(g.qz);
    const double coord = fmax(fmax(fabs((double)P.x), fabs((double)P.y)), fabs((double)P.z)) + nP;
    const double rr = (r * (1.0 + WIN_M_R) + WIN_M_COORD * coord) / (1.0 - WIN_M_LB); // LB (1 - M_LB) - M_COORD coord > r (1 + M_R)
    if (!(F2 > rr)) return 1 << 20;                                                   // LB(w) = F2 (w + 1) / (nP / iw + w + 1) never reaches it
    const double x = rr * (nP / fmax(iw, 1e-300)) / (F2 - rr);                        // LB(w) > rr  <=>  w + 1 > x
    return x < (double)(1 << 20) ? (int)x : 1 << 20;
}

