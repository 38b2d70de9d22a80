// CPU listing of the day-kernel selection in sng_step_plan.h (tests/test_day_lean_kernel_resources.py): one line
// per configuration, "N v2x noise legacy dt_pow2 packed req_stream req_zero diag lanes trajectory | step kernel
// name | day kernel name" (the last empty where the plan has no day kernel), over the same configurations as
// step_plan_check.cpp, each without and with SNG_GRAPH_TRAJECTORY.
#include <cstdio>

#include "sng_step_plan.h"

using namespace sng;

int main() {
    const int ns[] = {1, 2, 3, 4, 5, 8, 10, 16, 17, 50, 128};
    const int lanes[] = {1, 2, 4};
    char step[128], day[128];
    for (int n : ns)
        for (int bits = 0; bits < 256; ++bits)
            for (int l : lanes)
                for (int traj = 0; traj < 2; ++traj) {
                    if (!station_lanes_supported(n, l)) continue;
                    Params p{};
                    p.n = n;
                    p.v2x = (bits >> 7) & 1;
                    p.noise = (bits >> 6) & 1;
                    p.legacy = (bits >> 5) & 1;
                    p.dt_pow2 = (bits >> 4) & 1;
                    p.packed = (bits >> 3) & 1;
                    p.req_stream = (bits >> 2) & 1;
                    p.req_zero = (bits >> 1) & 1;
                    const bool diag = bits & 1;
                    p.lanes = l;
                    const StepPlan pl = step_plan(p, diag);
                    const int a = step_plan_name(pl, step, (int)sizeof step);
                    const int b = day_plan_name(pl, traj != 0, day, (int)sizeof day);
                    if (a <= 0 || a >= (int)sizeof step || b < 0 || b >= (int)sizeof day) return 1;
                    if ((b > 0) != (day_kernel_of(pl, traj != 0) != DAY_NONE)) return 2;
                    printf("%d %d %d %d %d %d %d %d %d %d %d | %s | %s\n", n, p.v2x, p.noise, p.legacy, p.dt_pow2,
                           p.packed, p.req_stream, p.req_zero, (int)diag, l, traj, step, day);
                }
    return 0;
}
