// win_index_check.cpp -- csrc/win_index.h held against / and % on the CPU (plain g++), for every candidate c < ncx * ncy of each window
// shape on the command line ("ncx ncy" pairs).  One line per shape: "ncx ncy wrong first_wrong_c" (first_wrong_c = -1: none).
// With "bare" as the first argument the split is the multiplication alone, as the wide-window passes took it before the header
// existed: the test that drives this program shows with it that the shapes can tell a wrong split from a right one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "win_index.h"

int main(int argc, char **argv) {
    int a = 1;
    const bool bare = argc > 1 && !strcmp(argv[1], "bare");
    if (bare) a++;
    if ((argc - a) % 2 != 0 || argc - a < 2) {
        fprintf(stderr, "usage: %s [bare] ncx ncy [ncx ncy ...]\n", argv[0]);
        return 2;
    }
    for (; a + 1 < argc; a += 2) {
        const int ncx = atoi(argv[a]), ncy = atoi(argv[a + 1]);
        const int64_t M = (int64_t)ncx * ncy;
        if (ncx < 1 || ncy < 1 || M >= (1ll << 31)) {
            fprintf(stderr, "%d x %d is outside the domain\n", ncx, ncy);
            return 2;
        }
        WinIndex w = win_index_make(ncx, ncy);
        if (bare) w.fix = 0;
        int64_t wrong = 0, first = -1;
        for (int c = 0; c < (int)M; c++) {
            int r, col;
            win_index_split(w, c, r, col);
            if (r != c / ncx || col != c % ncx) {
                if (first < 0) first = c;
                wrong++;
            }
        }
        printf("%d %d %lld %lld\n", ncx, ncy, (long long)wrong, (long long)first);
    }
    return 0;
}
