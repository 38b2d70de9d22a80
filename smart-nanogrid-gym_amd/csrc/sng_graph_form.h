// sng_graph_form.h -- the form of a captured graph of days (sng_graph.cpp), decided once: which node steps a day, whether
// the resets are generated beside the steps, and where day d's blocks lie in the caller's arrays.
//
// sng_step_plan.h decides per kernel (which step kernel, which day kernel); this header composes those answers into a
// graph.  graph_form is what capture_days builds before it captures anything, and nothing behind it decides again:
// launch_day (sng_kernels.hip) is told the DayNode.  Host only, no HIP types: it compiles with plain g++
// (tests/native/graph_shape_check.cpp lists every form on the CPU).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sng.h"
#include "sng_layout.h"
#include "sng_step_plan.h"

namespace sng {

// The step kernel writes the diagnostics (DIAG) when any SngInfo array other than the flags and the
// day return is given.
inline bool info_diag(const InfoPtrs &info) {
    return info.grid_power || info.p_charge || info.p_discharge || info.bess_soc || info.pen_vehicle ||
           info.pen_battery || info.grid_cost || info.total_cost || info.solar || info.bess_power ||
           info.bess_calc_power || info.nonexistent || info.bess_initial || info.charger_power || info.vehicle_soc;
}

// The form of a captured day with the MLP actor in the loop (sng_graph_create_policy).  Decided here and nowhere
// else.  POLICY_NODES: T x (policy_kernel node, step node), the step nodes being the plan's own step kernel.
// POLICY_FUSED: day_lean_policy_kernel<NC, PK, REQ> (sng_policy.h), the actor between the steps of the plan's lean day
// kernel, one node a day.  It exists where day_lean_kernel does and policy_day_compiled says so (zero scratch, zero
// VGPR spills: tests/test_policy_kernel_resources.py); the wide N = 10 and N = 50 plans, the general kernel's
// stations, any diagnostics and SNG_GRAPH_STEP_NODES (`step_nodes`) take nodes.  Where it exists it is the default
// only where its day measured shorter than the node form's by more than the node form's own spread
// (policy_day_faster; profiles/policy_day_ab.txt); SNG_GRAPH_POLICY_FUSED (`force`: A/B runs
// and tests) takes it wherever it is compiled.
enum PolicyDayForm : int { POLICY_NODES, POLICY_FUSED };
inline PolicyDayForm policy_day_form(const StepPlan &pl, bool trajectory, bool step_nodes, bool force = false) {
    if (step_nodes || day_kernel_of(pl, trajectory) != DAY_LEAN || !policy_day_compiled(pl.nc, pl.pk, pl.req))
        return POLICY_NODES;
    return (policy_day_faster(pl.nc) || force) ? POLICY_FUSED : POLICY_NODES;
}
// A policy made by sng_policy_create_net (policy_net_kernel, sng_policy_net.h) has no fused day: its actor is a
// workgroup of four wavefronts on 64 rows with up to 160 KB of LDS, which no day kernel's wavefront can carry between
// its steps.  Every plan takes nodes, T x (policy_net_kernel node, step node), whatever is forced.
inline PolicyDayForm policy_net_day_form(const StepPlan &, bool /*trajectory*/, bool /*step_nodes*/, bool /*force*/ = false) {
    return POLICY_NODES;
}
// A device-RNG reset is one launch -- the t = 0 observation as extra blocks of the generator's grid -- while the
// observation blocks' [kGenObsEnvs][obs_dim] LDS tile stays small next to the vehicle lists (32 KB: up to 60
// chargers); wider stations run profile_kernel and observe0_kernel behind the generator (launch_generate).
constexpr int kGenObsEnvs = 64;
inline bool generator_fused(const Params &p) { return (size_t)((kGenObsEnvs * p.obs_dim + 3) & ~3) * 4 <= 32 * 1024; }

// The shape of a captured reset graph (sng_graph_create with SNG_GRAPH_RESET).  Serial: every day's generator, then
// its steps, in one chain.  Overlapped: day d + 1 is generated into a second day slot while day d is stepped.
// Decided here and nowhere else, for a plan and a graph: at least two days, no kept trajectory (the generator
// would have to write every day's t = 0 observation; without one, step 0 overwrites that row, so the overlapped
// generator skips it), the one-launch generator, no SNG_GRAPH_SERIAL_RESET -- and a plan whose day measured
// shorter that way (device time per day at 65,536 envs, serial -> overlapped, profiles/overlapped_reset_ab.txt),
// whether its day is a day-kernel node or T step nodes:
//   - the wide family's 10-charger station: 93.3 -> 87.0 us (with the requested-SoC stream 126.3 -> 123.1).
// Not shorter, so serial unless forced (SNG_GRAPH_OVERLAPPED_RESET, `force`: A/B runs and tests):
//   - the lean family's 8 chargers: 119.6 -> 112.6 - 117.3 us between HIP events, but bench.py's wall time 0.4 -
//     1.2 % behind the parent's; 4 chargers 68.5 -> 70.8 us; 16 chargers 184.8 -> 240.2 us;
//   - config 5's 50 chargers, 2.12 -> 2.15 ms: its step kernel's eight wavefronts take a CU's whole LDS, so a
//     generator workgroup that gets in keeps a wavefront out;
//   - every plan that was not measured.
inline bool reset_overlapped(const StepPlan &pl, const Params &p, int days, bool trajectory, bool serial,
                             bool force = false) {
    const bool faster = pl.family == STEP_WIDE && pl.nc == 10;
    return days >= 2 && !trajectory && !serial && generator_fused(p) && (faster || force);
}
// The dynamic LDS an overlapped graph's generator workgroups ask for at least (bytes; 0: what they need).  Beside
// the wide family's day, which has exactly two wavefronts per SIMD to run and 40 KB of tiles per CU to place, the
// generator at its own eight wavefronts per SIMD doubled in length and stretched the day by more than the reset
// it hid (93.6 -> 101.6 us).  With 56 KB a workgroup, two fit a CU and leave the day's wavefronts their room:
// 85.5 us on that box (54 - 60 KB alike; 41 KB, three a CU: 93.6; 64 KB, which leaves 32 KB: 98.2).  The lean
// family's day is one wavefront per SIMD and was shorter beside the uncapped generator (N = 8: 114.9 us, capped
// 117.2 - 118.3), so a forced overlap there is not capped.
inline size_t overlapped_generator_lds(const StepPlan &pl) { return pl.family == STEP_WIDE ? 56u * 1024u : 0u; }
// The same beside day_station_kernel (station_day: the graph's days run that kernel), which stages its table rows
// behind its tiles: 5,880 B a wavefront, 6,400 B as a CU allocates LDS (blocks of 1,280 B), and eight of those fit a
// CU's 160 KB beside two generator workgroups of up to 55 KB.  Measured beside that kernel, device time per day
// (profiles/day_station_step_ab.txt): 56 KB 87.0 us (a CU holds seven of the day's wavefronts), 54 KB 76.1 - 77.3,
// 52 KB 86.0 - 87.1 (three generator workgroups fit a CU where they arrive first).
inline size_t overlapped_generator_lds(const StepPlan &pl, bool station_day) {
    return station_day ? 54u * 1024u : overlapped_generator_lds(pl);
}
// Day d of `days` in such a graph: the day slot it is generated into and stepped in (0: the handle's own
// buffers, 1: the shadow's -- the last day is always in slot 0, so after a replay the loaded day is where every
// other call expects it); the day index its generator draws, as an offset from the day counter at launch (the
// overlapped generators all read the counter before anything advances it); whether the day's first step advances
// the counter (Params::bump_day); and the amount a bump node behind the day's generator adds.  Per replay the
// counter advances by `days` in both forms.
struct DayShape { int slot, day_delta, bump_day, bump_node; };
inline DayShape day_shape(bool overlapped, int days, int d) {
    if (!overlapped) return {0, 0, 1, 0};
    const bool last = d == days - 1;
    return {(days - 1 - d) & 1, d, last ? 1 : 0, last ? days - 1 : 0};
}

// Day d's element offsets into the caller's arrays.  With a kept trajectory (SNG_GRAPH_TRAJECTORY) obs is [days][T + 1]
// [E][obs_dim] (block 0 of a day is the reset's observation), reward and done are [days][T][E] and a policy graph's
// actions_out is [days][T][E][act_dim]: obs0 is the day's first block, and obs_step / out_step / act_step lead from one
// step's block to the next.  Without one every step overwrites one block and all of them are 0.  noise_day is day d's
// block of a noise source's [days][T][E][act_dim] buffer, trajectory or not.
struct DayBlocks {
    // floats to the reset's observation block (step 0's is obs_step behind it), elements to step 0's reward and done,
    // floats to step 0's actions_out block and to the day's noise block
    size_t obs0, out, actions, noise_day;
    int64_t obs_step, out_step, act_step;
};
inline DayBlocks day_blocks(bool trajectory, int d, int T, int64_t E, int obs_dim, int act_dim) {
    const size_t obs_block = (size_t)E * (size_t)obs_dim, act_block = (size_t)E * (size_t)act_dim;
    const size_t steps = (size_t)d * (size_t)T;   // before day d
    if (!trajectory) return {0, 0, 0, steps * act_block, 0, 0, 0};
    return {(size_t)d * (size_t)(T + 1) * obs_block, steps * (size_t)E, steps * act_block, steps * act_block,
            (int64_t)obs_block, E, (int64_t)act_block};
}

// What takes the actions: the caller's stream of them, sng_policy_create's 64-64 actor or sng_policy_create_net's.
enum PolicyKind : int { POLICY_NONE, POLICY_MLP, POLICY_NET };
// The nodes that step one day: T step nodes of the plan's step kernel; one node of day_lean_kernel, day_wide_kernel or
// day_station_kernel; T x (actor node, step node); one node of day_lean_policy_kernel.
enum DayNode : int { DAY_STEP_NODES, DAY_KERNEL_LEAN, DAY_KERNEL_WIDE, DAY_KERNEL_STATION, DAY_POLICY_NODES, DAY_POLICY_FUSED };

struct GraphForm {
    StepPlan plan;
    bool with_reset, trajectory, overlapped;
    DayNode day;
    size_t generator_lds;       // overlapped: the dynamic LDS the generators ask for at least
    int nodes_per_day;          // the nodes that step a day (sng_graph_step_nodes), the reset's not counted
    char day_kernel_name[128];   // a day-kernel node's kernel as rocprofv3 names it (no policy); else empty
};

// The graph sng_graph_create* captures for a handle's Params (those of the day the graph steps), the SNG_GRAPH_* bits of
// `flags` and `days`:
//   - without a policy a day is one day-kernel node where the plan has one (day_kernel_of), else -- or with
//     SNG_GRAPH_STEP_NODES -- T step nodes; the wide plan's day kernel is the station-fixed one where the plan selects
//     it (day_station_selected), unless SNG_GRAPH_GENERIC_DAY keeps the generic one;
//   - with the 64-64 actor one fused node where the plan takes that form (policy_day_form), else T x (actor, step); a
//     net actor's days are always nodes (policy_net_day_form);
//   - only a graph without a policy generates its resets beside the steps (reset_overlapped).
inline GraphForm graph_form(const Params &p, bool diag, int flags, int days, PolicyKind policy) {
    auto has = [flags](int bit) { return (flags & bit) != 0; };
    const bool step_nodes = has(SNG_GRAPH_STEP_NODES), force_fused = has(SNG_GRAPH_POLICY_FUSED);
    GraphForm f{step_plan(p, diag), has(SNG_GRAPH_RESET), has(SNG_GRAPH_TRAJECTORY)};
    const DayFamily fam = day_kernel_of(f.plan, f.trajectory);
    if (policy == POLICY_NONE) {
        if (step_nodes || fam == DAY_NONE) f.day = DAY_STEP_NODES;
        else if (fam == DAY_LEAN) f.day = DAY_KERNEL_LEAN;
        else f.day = day_station_selected(f.plan, p, has(SNG_GRAPH_GENERIC_DAY)) ? DAY_KERNEL_STATION : DAY_KERNEL_WIDE;
    } else {
        const PolicyDayForm form = policy == POLICY_NET ? policy_net_day_form(f.plan, f.trajectory, step_nodes, force_fused)
                                                        : policy_day_form(f.plan, f.trajectory, step_nodes, force_fused);
        f.day = form == POLICY_FUSED ? DAY_POLICY_FUSED : DAY_POLICY_NODES;
    }
    f.overlapped = policy == POLICY_NONE && f.with_reset &&
                   reset_overlapped(f.plan, p, days, f.trajectory, has(SNG_GRAPH_SERIAL_RESET),
                                    has(SNG_GRAPH_OVERLAPPED_RESET));
    f.generator_lds = f.overlapped ? overlapped_generator_lds(f.plan, f.day == DAY_KERNEL_STATION) : 0;
    f.nodes_per_day = f.day == DAY_STEP_NODES ? p.T : f.day == DAY_POLICY_NODES ? 2 * p.T : 1;
    if (f.day == DAY_KERNEL_STATION) day_station_name(f.day_kernel_name, (int)sizeof f.day_kernel_name);
    else if (f.day == DAY_KERNEL_LEAN || f.day == DAY_KERNEL_WIDE)
        day_plan_name(f.plan, f.trajectory, f.day_kernel_name, (int)sizeof f.day_kernel_name);
    return f;
}

}  // namespace sng
