// CPU listing of the form a captured policy day takes (sng_graph_form.h, policy_day_form), for
// tests/test_policy_cpu.py: one line per configuration, "N v2x noise legacy dt_pow2 packed req_stream req_zero diag
// lanes trajectory step_nodes forced | step kernel name | fused or nodes | compiled or -", over the configurations
// of day_plan_check.cpp, each without and with SNG_GRAPH_STEP_NODES and SNG_GRAPH_POLICY_FUSED.  "compiled": the
// plan has day_lean_policy_kernel (whatever the flags).
#include <cstdio>

#include "sng_graph_form.h"

using namespace sng;

int main() {
    const int ns[] = {1, 2, 3, 4, 5, 8, 10, 16, 17, 50, 128};
    const int lanes[] = {1, 2, 4};
    char step[128];
    for (int n : ns)
        for (int bits = 0; bits < 256; ++bits)
            for (int l : lanes)
                for (int traj = 0; traj < 2; ++traj)
                    for (int nf = 0; nf < 4; ++nf) {
                        const int nodes = nf & 1, force = nf >> 1;
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
                        if (a <= 0 || a >= (int)sizeof step) return 1;
                        const PolicyDayForm form = policy_day_form(pl, traj != 0, nodes != 0, force != 0);
                        const bool compiled = day_kernel_of(pl, traj != 0) == DAY_LEAN && policy_day_compiled(pl.nc, pl.pk, pl.req);
                        // a fused day needs its kernel, never under SNG_GRAPH_STEP_NODES, always where it is asked for
                        if ((form == POLICY_FUSED) && (nodes || !compiled)) return 2;
                        if (force && !nodes && compiled && form != POLICY_FUSED) return 3;
                        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d | %s | %s | %s\n", n, p.v2x, p.noise, p.legacy,
                               p.dt_pow2, p.packed, p.req_stream, p.req_zero, (int)diag, l, traj, nodes, force, step,
                               form == POLICY_FUSED ? "fused" : "nodes", compiled ? "compiled" : "-");
                    }
    return 0;
}
