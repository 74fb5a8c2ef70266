// win_index.h -- candidate c of a pixel window, row-major, as (row, column): the one copy of that split, for the wave and the workgroup
// form of the cloud filter's wide-window passes (k_filter_win.hip: WinCand) and for the programs that hold it against / and %
// (tests/cpp/win_index_check.cpp with plain g++; rsm_stage_win_index_check on the device).
//
// DOMAIN: a window of ncx >= 1 columns and ncy >= 1 rows with M = ncx * ncy < 2^31, c in [0, M) -- every window win_clip can form: it is
// clipped to the lattice copy, whose cell count the filter keeps below 2^31 (whole_chip_search refuses more; M is an int).
//
// The row comes from a multiplication (the integer division was half of the wave kernel's instructions): with m = ceil(2^32 / ncx),
// m ncx = 2^32 + e, 0 <= e < ncx,
//     q = floor(c m / 2^32) = floor(c / ncx + c e / (ncx 2^32)).
// The second term is below c / 2^32 < 1/2 on the domain, so q is the row or the row plus one, and a negative column tells which: one
// correction step makes the split exact for EVERY window of the domain.  It is exact without the step when c e < 2^32 for all c < M,
// which M ncx <= 2^32 guarantees (e < ncx) -- windows up to ~1625 pixels a side; the constant says which case holds (wave-uniform: a
// property of the window), so the small windows, where nearly all queries are decided, keep the bare multiplication.
// (Before this header the bare multiplication served every window: the row was one too large, the column negative, for 1262 of the 2561
// rows' last candidates of an unclipped 1280-pixel window -- first at c = 3329299.)
#ifndef RSM_WIN_INDEX_H
#define RSM_WIN_INDEX_H

#include <stdint.h>

#if defined(__HIPCC__)
#define WIN_INDEX_FN __host__ __device__ __forceinline__
#else
#define WIN_INDEX_FN inline
#endif

struct WinIndex {
    int ncx;      // the window's row length
    uint32_t inv; // ceil(2^32 / ncx); 0 for ncx = 1 (it does not fit: the row is c itself)
    int fix;      // all ones: the multiplication alone may give row + 1, take the correction step; 0: it is exact
};

// the constant of a window of ncx x ncy candidates (the domain above)
WIN_INDEX_FN WinIndex win_index_make(int ncx, int ncy) {
    WinIndex w;
    w.ncx = ncx;
    w.inv = ncx > 1 ? 0xffffffffu / (uint32_t)ncx + 1u : 0u;
    w.fix = (uint64_t)ncx * (uint64_t)ncx * (uint64_t)ncy > (1ull << 32) ? -1 : 0;
    return w;
}

// row = c / ncx, col = c % ncx
WIN_INDEX_FN void win_index_split(const WinIndex &w, int c, int &row, int &col) {
#if defined(__HIP_DEVICE_COMPILE__)
    const int q = (int)__umulhi((unsigned int)c, w.inv);
#else
    const int q = (int)(((uint64_t)(uint32_t)c * (uint64_t)w.inv) >> 32);
#endif
    const int r = w.ncx > 1 ? q : c; // (ncx = 1: the reciprocal does not fit; a select, not a branch)
    const int cc = c - r * w.ncx;
    const int neg = (cc >> 31) & w.fix; // all ones: the multiplication gave row + 1 (no branch: the callers' loads stay in flight together)
    row = r + neg;
    col = cc + (w.ncx & neg);
}

#endif
