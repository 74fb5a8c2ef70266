// refine_plan_dump -- prints the refine schedule (csrc/refine_plan.h) of every case on stdin, one line each, for
// tests/test_refine_plan_cpu.py.  A case is one line of numbers in the order of FIELDS there:
//   W H ndir  YL0 YR0 XL0 XR0  YL1 YR1 XL1 XR1  iters top have_upd turn_px
//   skew_from skew_T skew_min_px skew_uw skew_rows skew_waves skew_waves_alone skew_waves_low
//   tile_T tile_from tile_min_px  rekey_until split  heavy_exclusive heavy_min_px heavy_from_sweep heavy_lanes
//   alone profiling second
// Output: "skewT skew_uw skew_rows zero_counters" and the steps: F (first sweep), B<lane> / E<lane> (turn begins / ends),
// K (fork), J (join), L:<S|W|T>:t:T:rf_launch:rekey:chains:timed (single / skewed / tile launch).
#include "refine_plan.h"

#include <stdio.h>

int main() {
    RefinePlanIn in{};
    int top, have_upd, alone, profiling, second;
    for (;;) {
        const int n = scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %lf %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &in.W, &in.H,
                            &in.ndir, &in.m[0].YL, &in.m[0].YR, &in.m[0].XL, &in.m[0].XR, &in.m[1].YL, &in.m[1].YR, &in.m[1].XL, &in.m[1].XR,
                            &in.iters, &top, &have_upd, &in.turn_px, &in.skew_from, &in.skew_T, &in.skew_min_px, &in.skew_uw, &in.skew_rows,
                            &in.skew_waves, &in.skew_waves_alone, &in.skew_waves_low, &in.tile_T, &in.tile_from, &in.tile_min_px,
                            &in.rekey_until, &in.split, &in.heavy_exclusive, &in.heavy_min_px, &in.heavy_from_sweep, &in.heavy_lanes, &alone,
                            &profiling, &second);
        if (n == EOF) return 0;
        if (n != 35) {
            fprintf(stderr, "refine_plan_dump: a case of %d fields\n", n);
            return 1;
        }
        in.top = top != 0;
        in.have_upd = have_upd != 0;
        in.alone = alone != 0;
        in.profiling = profiling != 0;
        in.second = second != 0;
        const RefinePlan p = refine_plan(in);
        printf("%d %d %d %d", p.skewT, p.skew_uw, p.skew_rows, (int)p.zero_counters);
        for (const RefineStep &s : p.steps) switch (s.kind) {
            case RS_FIRST: printf(" F"); break;
            case RS_TURN_BEGIN: printf(" B%d", s.lane); break;
            case RS_TURN_END: printf(" E%d", s.lane); break;
            case RS_FORK: printf(" K"); break;
            case RS_JOIN: printf(" J"); break;
            case RS_LAUNCH:
                printf(" L:%c:%d:%d:%d:%d:%d:%d", "SWT"[s.launch], s.t, s.T, s.rf_launch, (int)s.rekey, s.chains, (int)s.timed);
                break;
            }
        printf("\n");
    }
}
