// CPU listing of the step plan in sng_step_plan.h (tests/test_step_plan_cpu.py): one line per configuration,
// "N v2x noise legacy dt_pow2 packed req_stream req_zero diag lanes | kernel name", over every combination of
// the switches at a set of charger counts inside and outside the compiled station sizes, the multi-lane
// values only where step_lanes_per_env accepts them.  The test compares it with the listing of the library
// before the plan existed (tests/golden/step_kernel_names.json).
#include <cstdio>

#include "sng_step_plan.h"

using namespace sng;

int main() {
    const int ns[] = {1, 2, 3, 4, 5, 8, 10, 16, 17, 50, 128};
    const int lanes[] = {1, 2, 4};
    char name[128];
    for (int n : ns)
        for (int bits = 0; bits < 256; ++bits)
            for (int l : lanes) {
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
                const int len = step_plan_name(step_plan(p, diag), name, (int)sizeof name);
                if (len <= 0 || len >= (int)sizeof name) return 1;
                printf("%d %d %d %d %d %d %d %d %d %d | %s\n", n, p.v2x, p.noise, p.legacy, p.dt_pow2, p.packed,
                       p.req_stream, p.req_zero, (int)diag, l, name);
            }
    return 0;
}
