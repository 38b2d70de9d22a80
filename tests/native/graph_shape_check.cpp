// CPU listing of the captured graph's form in sng_graph_form.h (tests/test_graph_shape_cpu.py), over the same
// configurations as step_plan_check.cpp, with the dimensions of a bounded PV + BESS station on 1 h days (obs_dim =
// 2 N + 9, act_dim = N + 1, T = 24).
//
// Without arguments, the reset-graph shape:
//   plan N v2x noise legacy dt_pow2 packed req_stream req_zero diag lanes | step kernel name | fused lds | flags
// where `lds` is overlapped_generator_lds and `flags` holds reset_overlapped for days = 1 .. 5, each as eight
// digits: (trajectory, serial) = (0, 0), (0, 1), (1, 0), (1, 1) without SNG_GRAPH_OVERLAPPED_RESET, then with it; then, for both forms and days = 1 .. 5, one line per day of day_shape:
//   shape overlapped days d | slot day_delta bump_day bump_node
// then day_blocks for (trajectory, d, T, E) with the 10-charger station's dims (obs_dim 29, act_dim 11):
//   blocks trajectory d T E | obs0 obs_step out_step act_step out actions noise_day
//
// `graph_shape_check forms N`: graph_form for every configuration of N chargers, crossed with the policy kind, with
// and without SNG_GRAPH_RESET, every subset of the six other SNG_GRAPH_* bits and days = 1 .. 3.  Per configuration
//   cfg N v2x noise legacy dt_pow2 packed req_stream req_zero diag lanes | station kernel name | the plan's day kernel
//       name without a kept trajectory | with one
// and then one line of numbers per form: the inputs, every GraphForm field (the name as 0: empty, 1: the station
// kernel's, 2: the plan's for the form's trajectory), and the raw predicates graph_form composes:
//   policy with_reset bits days  with_reset trajectory overlapped day generator_lds nodes_per_day name
//   day_kernel_of day_station_selected policy_day_form reset_overlapped overlapped_generator_lds(plan) (plan, true)
// `bits`: 1 STEP_NODES, 2 TRAJECTORY, 4 SERIAL_RESET, 8 OVERLAPPED_RESET, 16 POLICY_FUSED, 32 GENERIC_DAY.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "sng_graph_form.h"

using namespace sng;

static const int kLanes[] = {1, 2, 4};

// configuration `bits` of N chargers at `l` lanes per env; false where the lane count is not supported
static bool configure(int n, int bits, int l, Params &p, bool &diag) {
    if (!station_lanes_supported(n, l)) return false;
    p = Params{};
    p.n = n;
    p.obs_dim = 2 * n + 9;
    p.act_dim = n + 1;
    p.T = 24;
    p.pv = p.bess = p.bounded = 1;
    p.v2x = (bits >> 7) & 1;
    p.noise = (bits >> 6) & 1;
    p.legacy = (bits >> 5) & 1;
    p.dt_pow2 = (bits >> 4) & 1;
    p.packed = (bits >> 3) & 1;
    p.req_stream = (bits >> 2) & 1;
    p.req_zero = (bits >> 1) & 1;
    diag = bits & 1;
    p.lanes = l;
    return true;
}

static int list_forms(int n) {
    const int flag_of[] = {SNG_GRAPH_STEP_NODES,       SNG_GRAPH_TRAJECTORY,   SNG_GRAPH_SERIAL_RESET,
                           SNG_GRAPH_OVERLAPPED_RESET, SNG_GRAPH_POLICY_FUSED, SNG_GRAPH_GENERIC_DAY};
    char station[128], name[2][128];
    for (int bits = 0; bits < 256; ++bits)
        for (int l : kLanes) {
            Params p;
            bool diag;
            if (!configure(n, bits, l, p, diag)) continue;
            const StepPlan pl = step_plan(p, diag);
            day_station_name(station, (int)sizeof station);
            for (int traj = 0; traj < 2; ++traj) day_plan_name(pl, traj != 0, name[traj], (int)sizeof name[traj]);
            printf("cfg %d %d %d %d %d %d %d %d %d %d | %s | %s | %s\n", n, p.v2x, p.noise, p.legacy, p.dt_pow2, p.packed,
                   p.req_stream, p.req_zero, (int)diag, l, station, name[0], name[1]);
            for (int policy = POLICY_NONE; policy <= POLICY_NET; ++policy)
                for (int reset = 0; reset < 2; ++reset)
                    for (int sub = 0; sub < 64; ++sub)
                        for (int days = 1; days <= 3; ++days) {
                            int flags = reset ? SNG_GRAPH_RESET : 0;
                            for (int k = 0; k < 6; ++k)
                                if (sub >> k & 1) flags |= flag_of[k];
                            const bool step_nodes = sub & 1, traj = sub & 2, serial = sub & 4, force_overlap = sub & 8,
                                       force_fused = sub & 16, generic = sub & 32;
                            const GraphForm f = graph_form(p, diag, flags, days, (PolicyKind)policy);
                            int which = 0;
                            if (f.day_kernel_name[0]) {
                                which = !strcmp(f.day_kernel_name, station) ? 1 : !strcmp(f.day_kernel_name, name[traj]) ? 2 : 3;
                                if (which == 3 || !strcmp(station, name[traj])) return 1;
                            }
                            const StepPlan &q = f.plan;   // the form carries the plan it was decided for
                            if (q.family != pl.family || q.nc != pl.nc || q.lanes != pl.lanes || q.pk != pl.pk ||
                                q.req != pl.req || q.noise != pl.noise || q.diag != pl.diag || q.fast != pl.fast)
                                return 1;
                            printf("%d %d %d %d %d %d %d %d %zu %d %d %d %d %d %d %zu %zu\n", policy, reset, sub, days,
                                   (int)f.with_reset, (int)f.trajectory, (int)f.overlapped, (int)f.day, f.generator_lds,
                                   f.nodes_per_day, which, (int)day_kernel_of(pl, traj),
                                   (int)day_station_selected(pl, p, generic),
                                   (int)policy_day_form(pl, traj, step_nodes, force_fused),
                                   (int)reset_overlapped(pl, p, days, traj, serial, force_overlap),
                                   overlapped_generator_lds(pl), overlapped_generator_lds(pl, true));
                        }
        }
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "forms")) return list_forms(atoi(argv[2]));
    const int ns[] = {1, 2, 3, 4, 5, 8, 10, 16, 17, 50, 128};
    char step[128];
    for (int n : ns)
        for (int bits = 0; bits < 256; ++bits)
            for (int l : kLanes) {
                Params p;
                bool diag;
                if (!configure(n, bits, l, p, diag)) continue;
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
    for (int traj = 0; traj < 2; ++traj)
        for (int d = 0; d < 3; ++d)
            for (int T : {12, 24})
                for (int E : {1, 96}) {
                    const DayBlocks b = day_blocks(traj != 0, d, T, E, 29, 11);
                    printf("blocks %d %d %d %d | %zu %lld %lld %lld %zu %zu %zu\n", traj, d, T, E, b.obs0,
                           (long long)b.obs_step, (long long)b.out_step, (long long)b.act_step, b.out, b.actions, b.noise_day);
                }
    return 0;
}
