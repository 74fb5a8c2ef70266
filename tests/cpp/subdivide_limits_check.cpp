// subdivide_limits_check.cpp -- csrc/subdivide_limits.h's size check against the same two inequalities in 128-bit arithmetic, at and around
// the boundaries 3 nf_out = 2^31 - 3, 2^31, 2^31 + 3 and nv_out = INT32_MAX, INT32_MAX + 1, for splits of nv_out into the vertices that
// were there and the edges that split, and for arguments large enough to wrap a 64-bit sum or product.  Plain g++ (tests/test_meshsubdivide_cpu.py
// builds and runs it); prints one line per case "nv_in n_split nf_out got want" and exits 1 when any differ.
#include "subdivide_limits.h"

#include <stdio.h>

typedef unsigned __int128 u128;

static int want(uint64_t nv_in, uint64_t n_split, uint64_t nf_out) {
    const u128 nv_out = (u128)nv_in + (u128)n_split;
    return nv_out <= (u128)INT32_MAX && (u128)3 * (u128)nf_out < ((u128)1 << 31) ? 1 : 0;
}

int main() {
    const uint64_t two31 = (uint64_t)1 << 31, imax = (uint64_t)INT32_MAX;
    // 2^31 = 2 (mod 3): no face count has 3 nf = 2^31 - 3, 2^31 or 2^31 + 3 exactly.  The counts on either side of each: 3 nf = 2^31 - 5 and
    // 2^31 - 2 (both taken; 715827882 is the largest), 2^31 + 1 (the first refused) and 2^31 + 4
    const uint64_t faces[] = {0, 1, (two31 - 5) / 3, (two31 - 2) / 3, (two31 + 1) / 3, (two31 + 4) / 3, two31, ~(uint64_t)0 / 3 + 1, ~(uint64_t)0};
    const uint64_t verts[] = {0, 1, imax - 1, imax, imax + 1, two31 + 5, ~(uint64_t)0 - 1, ~(uint64_t)0};
    int bad = 0, cases = 0, taken = 0;
    for (uint64_t nf_out : faces)
        for (uint64_t nv_out : verts) {
            // nv_out as nv_in + n_split in several ways, among them everything old, everything new, and a wrapping pair
            const uint64_t splits[] = {0, 1, nv_out / 2, nv_out > 0 ? nv_out - 1 : 0, nv_out};
            for (uint64_t n_split : splits) {
                const uint64_t nv_in = nv_out - n_split;
                const int got = subdivide_sizes_ok(nv_in, n_split, nf_out), w = want(nv_in, n_split, nf_out);
                printf("%llu %llu %llu %d %d\n", (unsigned long long)nv_in, (unsigned long long)n_split, (unsigned long long)nf_out, got, w);
                bad += got != w;
                taken += got;
                cases++;
            }
            // a pair whose 64-bit sum wraps to a small number
            const int got = subdivide_sizes_ok(~(uint64_t)0, nv_out + 2, nf_out);
            bad += got != 0;
            cases++;
        }
    // the named boundaries, spelled out
    bad += subdivide_sizes_ok(imax, 0, (two31 - 2) / 3) != 1;
    bad += subdivide_sizes_ok(imax - 7, 7, (two31 - 2) / 3) != 1;
    bad += subdivide_sizes_ok(imax - 7, 8, (two31 - 2) / 3) != 0;
    bad += subdivide_sizes_ok(imax, 1, 1) != 0;
    bad += subdivide_sizes_ok(1, 1, (two31 + 1) / 3) != 0;
    bad += subdivide_sizes_ok(1, 1, (two31 + 4) / 3) != 0;
    fprintf(stderr, "%d cases, %d taken, %d wrong\n", cases, taken, bad);
    return bad || taken == 0 || taken == cases ? 1 : 0;
}
