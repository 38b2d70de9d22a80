// CPU listing of the reset-graph shape in sng_step_plan.h (tests/test_graph_shape_cpu.py), over the same
// configurations as step_plan_check.cpp, with the observation row of a PV + BESS station (obs_dim = 2 N + 9):
//   plan N v2x noise legacy dt_pow2 packed req_stream req_zero diag lanes | step kernel name | fused lds | flags
// where `lds` is overlapped_generator_lds and `flags` holds reset_overlapped for days = 1 .. 5, each as eight
// digits: (trajectory, serial) = (0, 0), (0, 1), (1, 0), (1, 1) without SNG_GRAPH_OVERLAPPED_RESET, then with it; then, for both forms and days = 1 .. 5, one line per day of day_shape:
//   shape overlapped days d | slot day_delta bump_day bump_node
#include <cstdio>

#include "sng_step_plan.h"

using namespace sng;

int main() {
    const int ns[] = {1, 2, 3, 4, 5, 8, 10, 16, 17, 50, 128};
    const int lanes[] = {1, 2, 4};
    char step[128];
    for (int n : ns)
        for (int bits = 0; bits < 256; ++bits)
            for (int l : lanes) {
                if (!station_lanes_supported(n, l)) continue;
                Params p{};
                p.n = n;
                p.obs_dim = 2 * n + 9;
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
                if (a <= 0 || a >= (int)sizeof step) return 1;
                printf("plan %d %d %d %d %d %d %d %d %d %d | %s | %d %d |", n, p.v2x, p.noise, p.legacy, p.dt_pow2, p.packed,
                       p.req_stream, p.req_zero, (int)diag, l, step, (int)generator_fused(p),
                       (int)overlapped_generator_lds(pl));
                for (int days = 1; days <= 5; ++days) {
                    printf(" ");
                    for (int ts = 0; ts < 8; ++ts)
                        printf("%d", (int)reset_overlapped(pl, p, days, (ts & 2) != 0, (ts & 1) != 0, (ts & 4) != 0));
                }
                printf("\n");
            }
    for (int ov = 0; ov < 2; ++ov)
        for (int days = 1; days <= 5; ++days)
            for (int d = 0; d < days; ++d) {
                const DayShape s = day_shape(ov != 0, days, d);
                printf("shape %d %d %d | %d %d %d %d\n", ov, days, d, s.slot, s.day_delta, s.bump_day, s.bump_node);
            }
    return 0;
}
