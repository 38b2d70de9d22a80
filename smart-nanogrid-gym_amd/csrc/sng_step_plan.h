// sng_step_plan.h -- which step kernel a handle's Params select, and which day kernel a captured day of that plan
// runs (day_kernel_of), each decided once.  What a captured graph makes of these answers is sng_graph_form.h's.
//
// launch_step (sng_kernels.hip) dispatches the kernel a plan names and step_plan_name formats the same plan
// as the name rocprofv3 reports, so the two cannot disagree.  Host only, no HIP types: it compiles with plain
// g++ (tests/native/step_plan_check.cpp lists the name of every configuration on the CPU).
#pragma once
#include <stdio.h>

#include "sng_layout.h"

namespace sng {

// The station sizes the step kernels are compiled for: n, then whether step_lean_kernel<n, ...>,
// step_wide_kernel<n, kWideLanes, ...> and step_kernel<n, L, ...> with L = 2 and 4 lanes per env exist.  Any
// other charger count runs the general kernel with a runtime N (NC = 0), one lane per env.
struct StationSize {
    int n;
    bool lean, wide, lanes;
};
constexpr StationSize kStationSizes[] = {
    {1, true, false, false}, {2, true, false, true},  {4, true, false, true},  {8, true, false, true},
    {10, true, true, true},  {16, true, false, true}, {50, false, true, true},
};
inline const StationSize *station_size(int n) {
    for (const StationSize &s : kStationSizes)
        if (s.n == n) return &s;
    return nullptr;
}

// SngConfig.step_lanes_per_env (bench.py --lanes): one lane everywhere, two or four at the compiled sizes > 1.
inline bool station_lanes_supported(int n, int lanes) {
    const StationSize *s = station_size(n);
    return lanes == 1 || ((lanes == 2 || lanes == 4) && s && s->lanes);
}

// Lanes per env of the wide step kernel: two (2,048 wavefronts at 65,536 envs, two per SIMD).
// A/B at config 5 (round 3's tools/wide_ab.sh, in commits before 8be1f55; two runs each): 1 lane 25.85-25.91 us per step in the day graph,
// 2 lanes 22.54-22.62, 4 lanes 30.36-30.49 (128 VGPRs: 40 spilled to scratch).
constexpr int kWideLanes = 2;

enum StepFamily : int {
    STEP_LEAN,      // step_lean_kernel<NC, PK, REQ>
    STEP_WIDE,      // step_wide_kernel<NC, L, PK, REQ, NOISE>
    STEP_GENERAL,   // step_kernel<NC, L, DIAG, FAST, PK>
};

struct StepPlan {
    StepFamily family;
    int nc;      // compile-time charger count, 0 for a runtime N
    int lanes;   // lanes per env
    // the template flags (each family takes its own subset, above): the day is packed records (device-RNG days);
    // the requested-SoC stream is read; stochastic PV / price profiles; the SngInfo diagnostics are written;
    // NumPy-2 promotion with a power-of-two dt
    bool pk, req, noise, diag, fast;
};

// The lean and the wide kernel both take a compiled station, one lane per env as configured (they choose
// their own lanes), no diagnostics, and NumPy-2 promotion with a power-of-two dt.  Between them:
//   - the lean kernel (N <= 16, no stochastic profiles) is the default;
//   - stations of 10 chargers without V2X (the headline configuration) step through the wide kernel with two
//     lanes per env: A/B at 65,536 x 10 x 24 (round 3's tools/ab_headline.sh, in commits before 8be1f55; three runs each) 6.47-6.51 us per step
//     in the day graph vs 6.67-6.71 for the lean kernel, day 0.1749-0.1761 vs 0.1796-0.1803 ms; one lane per
//     env 6.75-6.79, four 8.15-8.23.  With V2X a discharging action is routine, and the lean kernel's LDS rows
//     keep numpy's order cheaper than the wide kernel's rolled re-read;
//   - N = 50 (BASELINE config 5's station) is the wide kernel's, stochastic profiles included.
// Everything else is the general kernel's: diagnostics, legacy promotion, another dt, a configured lane
// count of 2 or 4, stochastic profiles at N <= 16, a charger count that is not compiled in.
inline StepPlan step_plan(const Params &p, bool diag) {
    const StationSize *sz = station_size(p.n);
    const bool multi = p.lanes == 2 || p.lanes == 4, fast = !p.legacy && p.dt_pow2, noise = p.noise != 0;
    const bool special = sz && fast && !diag && !multi;
    StepPlan pl{STEP_GENERAL, sz ? p.n : 0, (multi && sz && sz->lanes) ? p.lanes : 1,
                p.packed != 0, p.req_stream && !p.req_zero, noise, diag, fast};
    if (special && sz->lean && !noise && (p.n != 10 || p.v2x)) {
        pl.family = STEP_LEAN;
    } else if (special && sz->wide && (p.n != 10 || (!noise && !p.v2x))) {
        pl.family = STEP_WIDE;
        pl.lanes = kWideLanes;
    }
    return pl;
}

// Which day kernel (sng_step_day.h) a plan has: a captured day's T steps as one launch.  Decided here and nowhere
// else: graph_form (sng_graph_form.h) asks this, and launch_day (sng_kernels.hip) launches what it decided.
//   - the lean family's plans run day_lean_kernel<NC, PK, REQ>, at every compiled lean size and for both timeline
//     encodings (but day_lean_compiled, below);
//   - the wide family's packed days at N = 10 run day_wide_kernel<10, 2, REQ, NOISE>.  That kernel keeps no
//     step's outputs but the last (it takes no per-step stride), so with `trajectory` the plan has none;
//   - N = 50 (it would spill), the wide family's unpacked days, the general kernel's plans and any plan with
//     diagnostics have none: their days stay T step nodes.
enum DayFamily : int { DAY_NONE, DAY_WIDE, DAY_LEAN };
// day_lean_kernel<nc, pk, req> is compiled for every lean size and flag pair but one: every instantiation must
// have zero scratch and zero VGPR spills (tests/test_day_lean_kernel_resources.py), and <1, true, true> -- one
// charger, packed days, the requested-SoC stream -- is left with a 36 B private segment by ROCm 7.2's LLVM (138
// VGPRs, 76 SGPR spills into VGPR lanes, no VGPR spill; a 32 B SGPR spill slot that no instruction uses survives
// frame lowering, whatever the occupancy attribute and the order of the loads).  Its plan keeps T step nodes.
constexpr bool day_lean_compiled(int nc, bool pk, bool req) { return !(nc == 1 && pk && req); }
inline DayFamily day_kernel_of(const StepPlan &pl, bool trajectory) {
    const StationSize *sz = station_size(pl.nc);
    if (pl.diag || !sz) return DAY_NONE;
    if (pl.family == STEP_LEAN && sz->lean) return day_lean_compiled(pl.nc, pl.pk, pl.req) ? DAY_LEAN : DAY_NONE;
    if (pl.family == STEP_WIDE && pl.pk && pl.lanes == kWideLanes && pl.nc == 10 && !trajectory) return DAY_WIDE;
    return DAY_NONE;
}
// Within DAY_WIDE: whether the day runs day_station_kernel<10, 2> (sng_step_day.h), day_wide_kernel<10, 2, false,
// false> with the station's switches as compile-time constants.  day_station_fixed is true exactly when every fact
// that kernel fixes holds for the handle: the wide family's packed days at N = 10 without the requested-SoC stream
// and without stochastic profiles (the plan), and PV, a BESS, bounded charging, no V2X, NumPy-2 promotion, a
// power-of-two dt, not a replayed day (req_zero: the cleared requests change req_default), the dimensions that
// follow from N with PV and a BESS -- and T = 24.  The kernel compares t + 1 with the constant for `done`, so another
// day length is not its station: the 2 h (T = 12) and 15 min (T = 96) days keep a power-of-two dt but go to the
// generic kernel, as every station that was not measured does (only the 1 h day was, profiles/day_station_kernel_ab.txt).
// A capture takes the station kernel where the predicate holds and its day measured shorter than the generic
// kernel's (day_station_faster), unless it asks for the generic one (`generic_day`, SNG_GRAPH_GENERIC_DAY: A/B runs
// and tests).
constexpr int kDayStationN = 10, kDayStationT = 24;
inline bool day_station_fixed(const StepPlan &pl, const Params &p) {
    return day_kernel_of(pl, false) == DAY_WIDE && pl.nc == kDayStationN && p.n == kDayStationN && !pl.req && !pl.noise &&
           !p.req_stream && !p.req_zero && !p.noise && p.packed && p.pv && p.bess && p.bounded && !p.v2x && !p.legacy &&
           p.dt_pow2 && p.T == kDayStationT && p.act_dim == kDayStationN + 1 && p.obs_dim == 2 * kDayStationN + 9;
}
constexpr bool day_station_faster() { return true; }
inline bool day_station_selected(const StepPlan &pl, const Params &p, bool generic_day) {
    return !generic_day && day_station_faster() && day_station_fixed(pl, p);
}
// The name rocprofv3 reports for the station kernel.
inline int day_station_name(char *buf, int len) {
    return snprintf(buf, (size_t)len, "void sng::day_station_kernel<%d, %d>", kDayStationN, kWideLanes);
}
// Whether day_lean_policy_kernel<NC, PK, REQ> (sng_policy.h), the lean day kernel with the MLP actor between its steps,
// is compiled for a plan (zero scratch, zero VGPR spills: tests/test_policy_kernel_resources.py) and whether its day
// measured shorter than T x (actor node, step node) (profiles/policy_day_ab.txt).  Which form a
// captured policy day takes is sng_graph_form.h's (policy_day_form).
constexpr bool policy_day_compiled(int nc, bool pk, bool req) { return day_lean_compiled(nc, pk, req); }
constexpr bool policy_day_faster(int /*nc*/) { return false; }

// The name rocprofv3 reports for a plan's day kernel; an empty string where it has none.
inline int day_plan_name(const StepPlan &pl, bool trajectory, char *buf, int len) {
    auto b = [](bool v) { return v ? "true" : "false"; };
    switch (day_kernel_of(pl, trajectory)) {
        case DAY_LEAN:
            return snprintf(buf, (size_t)len, "void sng::day_lean_kernel<%d, %s, %s>", pl.nc, b(pl.pk), b(pl.req));
        case DAY_WIDE:
            return snprintf(buf, (size_t)len, "void sng::day_wide_kernel<%d, %d, %s, %s>", pl.nc, pl.lanes, b(pl.req),
                            b(pl.noise));
        default: break;
    }
    return snprintf(buf, (size_t)len, "%s", "");
}

// The name rocprofv3 reports for a plan's kernel (bench.py looks its kernel-stats and PMC records up by it).
inline int step_plan_name(const StepPlan &pl, char *buf, int len) {
    auto b = [](bool v) { return v ? "true" : "false"; };
    if (pl.family == STEP_LEAN)
        return snprintf(buf, (size_t)len, "void sng::step_lean_kernel<%d, %s, %s>", pl.nc, b(pl.pk), b(pl.req));
    if (pl.family == STEP_WIDE)
        return snprintf(buf, (size_t)len, "void sng::step_wide_kernel<%d, %d, %s, %s, %s>", pl.nc, pl.lanes,
                        b(pl.pk), b(pl.req), b(pl.noise));
    return snprintf(buf, (size_t)len, "void sng::step_kernel<%d, %d, %s, %s, %s>", pl.nc, pl.lanes, b(pl.diag),
                    b(pl.fast), b(pl.pk));
}

}  // namespace sng
